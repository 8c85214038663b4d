"""The beam-search statement of DESIGN.md section 4 ("Beam search"), in float64 numpy.

CTC prefix beam search without a language model (Graves 2012, Hannun 2014; keras.backend.ctc_decode(greedy=False)) on
log q_t of tests/ctc_statement.py.  The beam is a dict prefix -> (log p_blank, log p_nonblank), starting from {(): (0, -inf)}.
Per frame every prefix proposes itself (blank, or a repeat of its last label) and its extension by each of the
E = min(beam_width, C - 1) non-blank classes of the largest `rank` value (ties: the smaller class; `rank` is log q_t itself
unless the caller gives the logits, which order the classes the same way) -- this pruning is part of the algorithm.  Proposals
that spell the same prefix are merged (log-add); those of total -inf are dropped; the best beam_width by total
lse(p_blank, p_nonblank) survive.  Tie rule: the higher total first, then the lexicographically smaller label row, -1 (the
padding) sorting after every label.  After the last frame the top_paths best prefixes are rescored with
ctc_statement.ctc_loss_logq (the exact sum over all alignments) and returned in the order of the rescored value (same tie rule).

Decision margin of a crop: the smallest gap met at any decision that floating-point error could turn -- per frame between
the last kept and the best dropped candidate and between the last kept and the first dropped class of the pruning; at the
end between the last returned and the best not returned prefix; between neighbouring returned paths' rescored values.  Each
gap is divided by max(1, |a|, |b|) of the two values compared, so that it reads against a relative error bound.  +inf where
nothing was ever dropped.
"""
import numpy as np

from tests import ctc_statement as cs

_AFTER = 1 << 30  # the padding's place in the row order: after every label


def row_key(prefix, width):
    return tuple(prefix) + (_AFTER,) * (width - len(prefix))


def _gap(a, b):
    return (a - b) / max(1.0, abs(a), abs(b))


def beam_search(lq, beam_width, top_paths, rank=None):
    """lq (T, C) float64 log q_t (blank = C - 1) -> (labels (top_paths, T) int64 -1 padded, log_prob (top_paths,) float64,
    -inf behind the paths that exist, margin float)."""
    lq = np.asarray(lq, np.float64)
    T, C = lq.shape
    blank = C - 1
    rank = lq if rank is None else np.asarray(rank, np.float64)
    E = min(beam_width, C - 1)
    beam = {(): (0.0, -np.inf)}
    margin = np.inf
    for t in range(T):
        order = sorted(range(C - 1), key=lambda c: (-rank[t, c], c))
        if E < C - 1:
            margin = min(margin, _gap(rank[t, order[E - 1]], rank[t, order[E]]))
        cand = {}

        def add(p, pb, pnb):
            old = cand.get(p, (-np.inf, -np.inf))
            cand[p] = (np.logaddexp(old[0], pb), np.logaddexp(old[1], pnb))

        for p, (pb, pnb) in beam.items():
            tot = np.logaddexp(pb, pnb)
            add(p, tot + lq[t, blank], pnb + lq[t, p[-1]] if p else -np.inf)
            for c in order[:E]:
                add(p + (c,), -np.inf, (pb if p and p[-1] == c else tot) + lq[t, c])
        ranked = sorted(((np.logaddexp(pb, pnb), row_key(p, T), p) for p, (pb, pnb) in cand.items()), key=lambda r: (-r[0], r[1]))
        ranked = [r for r in ranked if r[0] > -np.inf]
        if len(ranked) > beam_width:
            margin = min(margin, _gap(ranked[beam_width - 1][0], ranked[beam_width][0]))
        beam = {p: cand[p] for _, _, p in ranked[:beam_width]}
    ranked = sorted(((np.logaddexp(pb, pnb), row_key(p, T), p) for p, (pb, pnb) in beam.items()), key=lambda r: (-r[0], r[1]))
    if len(ranked) > top_paths:
        margin = min(margin, _gap(ranked[top_paths - 1][0], ranked[top_paths][0]))
    paths = [p for _, _, p in ranked[:top_paths]]
    rows = np.full((len(paths), T), -1, np.int64)
    for k, p in enumerate(paths):
        rows[k, :len(p)] = p
    logp = -cs.ctc_loss_logq(np.broadcast_to(lq, (len(paths), T, C)), rows, [len(p) for p in paths], [T] * len(paths))
    final = sorted(range(len(paths)), key=lambda k: (-logp[k], row_key(paths[k], T)))
    for a, b in zip(final, final[1:]):
        margin = min(margin, _gap(logp[a], logp[b]))
    labels = np.full((top_paths, T), -1, np.int64)
    log_prob = np.full(top_paths, -np.inf)
    labels[:len(final)] = rows[final]
    log_prob[:len(final)] = logp[final]
    return labels, log_prob, float(margin)


def beam_search_batch(lq, beam_width, top_paths, rank=None):
    """(M, T, C) -> labels (M, top_paths, T), log_prob (M, top_paths), margin (M,)."""
    out = [beam_search(lq[m], beam_width, top_paths, None if rank is None else rank[m]) for m in range(len(lq))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def all_labellings(y_pred):
    """Every labelling of one sample (y_pred (T, C) probabilities) that has an alignment, with its exact log-probability
    (ctc_statement.brute_force, the sum over all C**T paths): a list of (log_prob, label tuple) in the statement's order."""
    import itertools

    T, C = np.shape(y_pred)
    labs = sorted({tuple(cs.collapse(path, C - 1)) for path in itertools.product(range(C), repeat=T)})
    scored = [(-cs.brute_force(y_pred, lab, T), lab) for lab in labs]
    return sorted(scored, key=lambda r: (-r[0], row_key(r[1], T)))
