"""The pattern statement of DESIGN.md section 4 ("Patterns: the statement and its status"), in float64 numpy.

For a crop, ``lq`` is the To x C table of ctc_statement.log_q (blank = C - 1): the values lexicon_logq_kernel writes, all finite.
A pattern is a deterministic automaton: ``delta[S][C - 1]`` (-1: no move), ``accept[S]``, start state 0, trimmed.

  node        (s, blank), or (s, c) with c a label for which some p has delta[p][c] == s
  node order  state ascending; within a state the blank node first, then labels ascending
  recursion   V_0 = 0 at (0, blank), -inf elsewhere.  At frame t, (s, blank) takes the best of itself, then every (s, c);
              (s, c) takes the best of itself (repeat), then for every p with delta[p][c] == s the node (p, blank) and every
              (p, c') with c' != c; then lq[t][blank] or lq[t][c] is added
  tie rule    candidates in the order: stay, then predecessors in node order; the FIRST of the largest wins.  At the end the
              first of the largest among the accepting nodes.  ``last=True`` is the OPPOSITE rule (the last of the largest).
  result      log_path, the best end value; labels, the collapse of the traced-back alignment; (-inf, None) when no accepting
              node is reachable in To frames
  log_prob    -ctc_loss(labels) on the same lq: every alignment of that text (the all-blank path for the empty text)
  runner_up   the best log_path over accepted texts other than ``labels``: the pattern times the automaton "not this string"
  margin      log_path - runner_up; a (crop, pattern) pair is decidable when it exceeds 2 GATE To max(1, |log_path|)"""
import numpy as np

from tests import ctc_statement as cs

GATE = 1e-6  # tests/test_ctc_loss_gpu.py


def nodes_of(delta):
    """the nodes [(s, c)] in node order, c = -1 for the blank node, and per node its candidates' node indices in the
    statement's order (itself first)"""
    delta = np.asarray(delta)
    S, K = delta.shape
    enter = [[[] for _ in range(K)] for _ in range(S)]  # enter[s][c]: the p with delta[p][c] == s, ascending
    for p in range(S):
        for c in range(K):
            if delta[p, c] >= 0:
                enter[delta[p, c]][c].append(p)
    nodes, first = [], []
    for s in range(S):
        first.append(len(nodes))
        nodes.append((s, -1))
        nodes += [(s, c) for c in range(K) if enter[s][c]]
    first.append(len(nodes))
    cands = []
    for i, (s, c) in enumerate(nodes):
        if c < 0:
            cands.append(np.array([i] + list(range(first[s] + 1, first[s + 1])), np.int64))
        else:
            cand = [i]
            for p in enter[s][c]:
                cand += [j for j in range(first[p], first[p + 1]) if nodes[j][1] != c]
            cands.append(np.array(cand, np.int64))
    return nodes, cands


def _pick(values, last):
    """the index of the first (last) of the largest"""
    return int(len(values) - 1 - np.argmax(values[::-1])) if last else int(np.argmax(values))


def viterbi(lq, delta, accept, last=False):
    """(log_path, labels as a list) or (-inf, None)"""
    lq = np.asarray(lq, np.float64)
    To, C = lq.shape
    nodes, cands = nodes_of(delta)
    col = np.array([C - 1 if c < 0 else c for _, c in nodes])
    V = np.full(len(nodes), -np.inf)
    V[0] = 0.0
    back = np.zeros((To, len(nodes)), np.int64)
    for t in range(To):
        new = np.empty_like(V)
        for i, cand in enumerate(cands):
            k = _pick(V[cand], last)
            back[t, i] = cand[k]
            new[i] = V[cand[k]]
        V = new + lq[t, col]
    ends = np.array([i for i, (s, _) in enumerate(nodes) if accept[s]], np.int64)
    if not len(ends) or np.max(V[ends]) == -np.inf:
        return -np.inf, None
    node = int(ends[_pick(V[ends], last)])
    best, path = float(V[node]), []
    for t in range(To - 1, -1, -1):
        path.append(col[node])
        node = int(back[t, node])
    return best, cs.collapse(path[::-1], C - 1)


def log_prob(lq, labels):
    """-ctc_loss of the text on lq (To, C)"""
    lq = np.asarray(lq, np.float64)
    lab = np.asarray(list(labels) + [0], np.int64)[None]
    return float(-cs.ctc_loss_logq(lq[None], lab, [len(labels)], [lq.shape[0]])[0])


def product_without(delta, accept, labels, same=None):
    """the automaton of the pattern's texts other than ``labels`` (``same``: class -> its representative; a text that differs
    from ``labels`` only within the tie classes counts as ``labels``): (delta, accept), reachable states only, or None when
    nothing is left"""
    delta = np.asarray(delta)
    K = delta.shape[1]
    rep = (lambda c: c) if same is None else (lambda c: same.get(c, c))
    want = [rep(int(c)) for c in labels]
    L = len(want)
    index, order, rows = {(0, 0): 0}, [(0, 0)], []
    k = 0
    while k < len(order):
        s, pos = order[k]
        row = [-1] * K
        for c in range(K):
            t = int(delta[s, c])
            if t < 0:
                continue
            nxt = (t, pos + 1 if 0 <= pos < L and rep(c) == want[pos] else -1)
            if nxt not in index:
                index[nxt] = len(order)
                order.append(nxt)
            row[c] = index[nxt]
        rows.append(row)
        k += 1
    acc = [bool(accept[s]) and pos != L for s, pos in order]
    if not any(acc):
        return None
    return np.asarray(rows, np.int64).reshape(len(order), K), acc


def runner_up(lq, dfa, labels, same=None):
    """the best log_path over the accepted texts other than ``labels`` (-inf: there is none that fits)"""
    rest = product_without(dfa[0], dfa[1], labels, same)
    return -np.inf if rest is None else viterbi(lq, rest[0], rest[1])[0]


def next_value(lq, delta, accept):
    """the largest log_path of an accepted ALIGNMENT that is strictly below the best one (-inf: none): what an exact tie's
    winners are apart from everything that is not tied with them.  The same recursion on the two largest distinct values."""
    lq = np.asarray(lq, np.float64)
    To, C = lq.shape
    nodes, cands = nodes_of(delta)
    col = np.array([C - 1 if c < 0 else c for _, c in nodes])
    V = np.full((2, len(nodes)), -np.inf)
    V[0, 0] = 0.0
    for t in range(To):
        new = np.full_like(V, -np.inf)
        for i, cand in enumerate(cands):
            vals = V[:, cand].ravel()
            new[0, i] = vals.max()
            below = vals[vals < new[0, i]]
            if len(below):
                new[1, i] = below.max()
        V = new + lq[t, col]
    ends = [i for i, (s, _) in enumerate(nodes) if accept[s]]
    vals = V[:, ends].ravel()
    below = vals[vals < vals.max()]
    return float(below.max()) if len(below) else -np.inf


def bound(frames, log_path):
    return 2 * GATE * frames * max(1.0, abs(log_path))


def margin(lq, dfa, same=None):
    """(log_path, labels, margin): margin = log_path - runner_up, +inf when nothing else fits; None without a fit"""
    value, labels = viterbi(lq, dfa[0], dfa[1])
    if labels is None:
        return value, None, None
    return value, labels, value - runner_up(lq, dfa, labels, same)


def decidable(lq, dfa, same=None):
    value, labels, m = margin(lq, dfa, same)
    return labels is not None and m > bound(np.asarray(lq).shape[0], value)
