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


def _cut(values, n, stats):
    """The cut behind the n-th of `values` (sorted, largest first) for the tie-aware margin: a gap of exactly zero is an exact
    tie, which the tie rule decides and no rounding can turn -- it is counted, and the margin is then what separates the tied
    value from its nearest different neighbours on either side of it."""
    if len(values) <= n:
        return
    v = values[n - 1]
    if values[n] != v:
        stats["margin"] = min(stats["margin"], _gap(v, values[n]))
        return
    stats["ties"] += 1
    above = [x for x in values[:n] if x > v]
    below = [x for x in values[n:] if x < v]
    if above:
        stats["margin"] = min(stats["margin"], _gap(above[-1], v))
    if below:
        stats["margin"] = min(stats["margin"], _gap(v, below[0]))


def _ranked(entries, T, larger_row_first):
    sign = -1 if larger_row_first else 1
    rows = [(np.logaddexp(pb, pnb), tuple(sign * x for x in row_key(p, T)), p) for p, (pb, pnb) in entries.items()]
    return [r for r in sorted(rows, key=lambda r: (-r[0], r[1])) if r[0] > -np.inf]


def beam_frames(lq, beam_width, rank=None, larger_class_first=False, larger_row_first=False):
    """The frames of the search alone: (the final beam {prefix: (log p_blank, log p_nonblank)}, stats).  stats: "plain" the
    margin of the module docstring so far; "margin" / "ties" the same with exact ties counted instead of read as a zero
    margin (_cut); "lead" the smallest gap per frame between the best and the second-best candidate.
    larger_class_first / larger_row_first turn the tie rule of the class pruning / of the ranking round: the OPPOSITE rules,
    for showing that an input's answer hangs on the rule."""
    lq = np.asarray(lq, np.float64)
    T, C = lq.shape
    blank = C - 1
    rank = lq if rank is None else np.asarray(rank, np.float64)
    E = min(beam_width, C - 1)
    beam = {(): (0.0, -np.inf)}
    stats = {"plain": np.inf, "margin": np.inf, "ties": 0, "lead": np.inf}
    for t in range(T):
        order = sorted(range(C - 1), key=lambda c: (-rank[t, c], -c if larger_class_first else c))
        if E < C - 1:
            stats["plain"] = min(stats["plain"], _gap(rank[t, order[E - 1]], rank[t, order[E]]))
            _cut([rank[t, c] for c in order], E, stats)
        cand = {}

        def add(p, pb, pnb):
            old = cand.get(p, (-np.inf, -np.inf))
            cand[p] = (np.logaddexp(old[0], pb), np.logaddexp(old[1], pnb))

        for p, (pb, pnb) in beam.items():
            tot = np.logaddexp(pb, pnb)
            add(p, tot + lq[t, blank], pnb + lq[t, p[-1]] if p else -np.inf)
            for c in order[:E]:
                add(p + (c,), -np.inf, (pb if p and p[-1] == c else tot) + lq[t, c])
        ranked = _ranked(cand, T, larger_row_first)
        if len(ranked) > beam_width:
            stats["plain"] = min(stats["plain"], _gap(ranked[beam_width - 1][0], ranked[beam_width][0]))
        _cut([r[0] for r in ranked], beam_width, stats)
        if len(ranked) > 1:
            stats["lead"] = min(stats["lead"], _gap(ranked[0][0], ranked[1][0]))
        beam = {p: cand[p] for _, _, p in ranked[:beam_width]}
    return beam, stats


def beam_paths(lq, beam, top_paths, stats, larger_row_first=False):
    """The end of the search on beam_frames' result: (labels, log_prob) as beam_search returns them; a copy of `stats`
    brought up to date with the final ranking's decisions is returned as the third value."""
    lq = np.asarray(lq, np.float64)
    T, C = lq.shape
    stats = dict(stats)
    sign = -1 if larger_row_first else 1
    ranked = _ranked(beam, T, larger_row_first)
    if len(ranked) > top_paths:
        stats["plain"] = min(stats["plain"], _gap(ranked[top_paths - 1][0], ranked[top_paths][0]))
    _cut([r[0] for r in ranked], top_paths, stats)
    if len(ranked) > 1:
        stats["lead"] = min(stats["lead"], _gap(ranked[0][0], ranked[1][0]))
    paths = [p for _, _, p in ranked[:top_paths]]
    rows = np.full((len(paths), T), -1, np.int64)
    for k, p in enumerate(paths):
        rows[k, :len(p)] = p
    logp = -cs.ctc_loss_logq(np.broadcast_to(lq, (len(paths), T, C)), rows, [len(p) for p in paths], [T] * len(paths))
    final = sorted(range(len(paths)), key=lambda k: (-logp[k], tuple(sign * x for x in row_key(paths[k], T))))
    for i, (a, b) in enumerate(zip(final, final[1:])):
        stats["plain"] = min(stats["plain"], _gap(logp[a], logp[b]))
        if logp[a] == logp[b]:
            stats["ties"] += 1
        else:
            stats["margin"] = min(stats["margin"], _gap(logp[a], logp[b]))
        if i == 0:
            stats["lead"] = min(stats["lead"], _gap(logp[a], logp[b]))
    labels = np.full((top_paths, T), -1, np.int64)
    log_prob = np.full(top_paths, -np.inf)
    labels[:len(final)] = rows[final]
    log_prob[:len(final)] = logp[final]
    return labels, log_prob, stats


def beam_search(lq, beam_width, top_paths, rank=None):
    """lq (T, C) float64 log q_t (blank = C - 1) -> (labels (top_paths, T) int64 -1 padded, log_prob (top_paths,) float64,
    -inf behind the paths that exist, margin float)."""
    beam, stats = beam_frames(lq, beam_width, rank)
    labels, log_prob, stats = beam_paths(lq, beam, top_paths, stats)
    return labels, log_prob, float(stats["plain"])


def beam_search_ties(lq, beam_width, top_paths, rank=None, larger_class_first=False, larger_row_first=False):
    """beam_search for inputs with exact ties -> (labels, log_prob, stats): stats["margin"] is the decision margin with every
    gap between two values that compare EQUAL in float64 left out -- such a pair is an exact tie, decided by the tie rule on
    both sides, and is counted in stats["ties"] instead; stats["lead"] is the lead margin, the smallest gap over the frames
    and the final ranking between the best and the second-best candidate (what row 0 alone hangs on)."""
    beam, stats = beam_frames(lq, beam_width, rank, larger_class_first, larger_row_first)
    return beam_paths(lq, beam, top_paths, stats, larger_row_first)


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
