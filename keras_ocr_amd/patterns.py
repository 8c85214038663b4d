"""Patterns ("Patterns"): named regular expressions over a recogniser's alphabet that a crop may be
decoded under -- a date, an amount, a plate -- compiled on the host into the deterministic automata
``Context.set_patterns`` loads.

Syntax: literal characters of the alphabet; ``\\`` + character for a literal metacharacter; ``\\d`` (the alphabet's digits);
``.`` (any alphabet character); ``[...]`` with ranges and ``^`` negation; ``( )``, ``(?: )`` and ``|``; ``*``, ``+``, ``?``,
``{m}``, ``{m,}``, ``{m,n}``.  The match is always a full match: for every text over the alphabet, acceptance equals
``re.fullmatch(regex, text) is not None``.  Anything else -- anchors, backreferences, look-around, lazy or possessive
quantifiers, flags -- is a ValueError naming the pattern and the position.

Construction: regex -> NFA -> subset construction -> trim -> Moore minimisation; the states are renumbered breadth-first from
the start, labels ascending, so two spellings of one language give equal tables."""
import re

import numpy as np

MAX_PATTERNS = 64  # include/kocr.h: KOCR_PATTERNS_MAX
MAX_STATES = 256  # KOCR_PATTERN_MAX_STATES
MAX_NODES = 4096  # KOCR_PATTERN_MAX_NODES
MAX_REPEAT = 4096  # the largest count in {m,n}: far beyond what MAX_STATES admits, small enough to expand


class _Parser:
    """Recursive descent over one regex; the tree: ("set", frozenset of labels), ("cat", [nodes]), ("alt", [nodes]),
    ("rep", node, m, n or None)"""

    def __init__(self, name, regex, alphabet, lowercase):
        self.name, self.s, self.i = name, regex, 0
        self.alphabet, self.lowercase = alphabet, lowercase
        self.code = {ch: c for c, ch in enumerate(alphabet)}
        self.digits = frozenset(c for c, ch in enumerate(alphabet) if re.fullmatch(r"\d", ch))
        self.any = frozenset(c for c, ch in enumerate(alphabet) if re.fullmatch(r".", ch))

    def fail(self, what, at=None):
        raise ValueError(f"pattern {self.name!r}: {what} at position {self.i if at is None else at} of {self.s!r}")

    def peek(self):
        return self.s[self.i] if self.i < len(self.s) else ""

    def literal(self, ch, at):
        if self.lowercase:
            ch = ch.lower()
        if ch not in self.code:
            raise ValueError(f"pattern {self.name!r}: the alphabet cannot spell the character {ch!r} (position {at} of {self.s!r})")
        return self.code[ch]

    def parse(self):
        node = self.alt()
        if self.i < len(self.s):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        parts = []
        while self.peek() not in ("", "|", ")"):
            parts.append(self.repeat())
        return ("cat", parts)

    def repeat(self):
        if self.peek() in ("*", "+", "?", "{"):
            self.fail("nothing to repeat")
        node = self.atom()
        quantified = False
        while self.peek() in ("*", "+", "?", "{"):
            if quantified:
                self.fail("a quantifier behind a quantifier (lazy, possessive and repeated quantifiers are not supported)")
            ch = self.peek()
            if ch == "{":
                m = re.compile(r"\{(\d+)(?:(,)(\d*))?\}").match(self.s, self.i)
                if not m:
                    self.fail("'{' that does not open {m}, {m,} or {m,n} (a literal brace is written \\{)")
                lo = int(m.group(1))
                hi = lo if m.group(2) is None else (None if m.group(3) == "" else int(m.group(3)))
                if lo > MAX_REPEAT or (hi is not None and hi > MAX_REPEAT):
                    self.fail(f"a repetition count above {MAX_REPEAT}")
                if hi is not None and hi < lo:
                    self.fail("a repetition {m,n} with n < m")
                self.i = m.end()
            else:
                lo, hi = {"*": (0, None), "+": (1, None), "?": (0, 1)}[ch]
                self.i += 1
            node = ("rep", node, lo, hi)
            quantified = True
        return node

    def escape(self):
        """behind a backslash: the set it stands for"""
        at = self.i - 1
        ch = self.peek()
        if ch == "":
            self.fail("a backslash at the end", at)
        self.i += 1
        if ch == "d":
            return self.digits
        if ch.isalnum():
            self.fail(f"the escape \\{ch} is not supported (only \\d and escaped punctuation; no backreferences, anchors or "
                      f"other classes)", at)
        return frozenset([self.literal(ch, at)])

    def atom(self):
        at, ch = self.i, self.peek()
        self.i += 1
        if ch == "(":
            if self.peek() == "?":
                if self.s[self.i:self.i + 2] != "?:":
                    self.fail("a group extension other than (?: ) (no look-around, flags, names or conditionals)", at)
                self.i += 2
            node = self.alt()
            if self.peek() != ")":
                self.fail("a '(' that is never closed", at)
            self.i += 1
            return node
        if ch == "[":
            return ("set", self.char_class(at))
        if ch == ".":
            return ("set", self.any)
        if ch == "\\":
            return ("set", self.escape())
        if ch in ("^", "$"):
            self.fail(f"the anchor {ch!r} is not supported (the match is always a full match)", at)
        return ("set", frozenset([self.literal(ch, at)]))

    def char_class(self, at):
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        members, first = set(), True
        while True:
            ch = self.peek()
            if ch == "":
                self.fail("a '[' that is never closed", at)
            if ch == "]" and not first:
                self.i += 1
                break
            first = False
            lo_at = self.i
            self.i += 1
            if ch == "\\":
                lo = self.escape()
                single = None if len(lo) != 1 or self.s[lo_at + 1] == "d" else self.s[lo_at + 1]
            else:
                lo, single = None, ch
            if self.peek() == "-" and self.s[self.i + 1:self.i + 2] not in ("", "]"):
                if single is None:
                    self.fail("a range that starts with a class", lo_at)
                self.i += 1
                hi_at, hi = self.i, self.peek()
                self.i += 1
                if hi == "\\":
                    hi = self.peek()
                    if hi == "" or hi.isalnum():
                        self.fail("a range that ends with a class or an unsupported escape", hi_at)
                    self.i += 1
                a, b = (single.lower(), hi.lower()) if self.lowercase else (single, hi)
                if ord(a) > ord(b):
                    self.fail(f"the bad character range {a}-{b}", lo_at)
                members.update(c for c, x in enumerate(self.alphabet) if len(x) == 1 and ord(a) <= ord(x) <= ord(b))
            elif lo is not None:
                members.update(lo)
            else:
                members.add(self.literal(single, lo_at))
        return frozenset(set(range(len(self.alphabet))) - members) if negate else frozenset(members)


class _Nfa:
    def __init__(self):
        self.eps, self.moves = [], []  # per state: the epsilon targets; (set of labels, target)

    def state(self):
        self.eps.append([])
        self.moves.append([])
        return len(self.eps) - 1

    def build(self, node):
        """(start, end) of the fragment for ``node``"""
        kind = node[0]
        if kind == "set":
            a, b = self.state(), self.state()
            self.moves[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.state()
            for part in node[1]:
                s, e = self.build(part)
                self.eps[b].append(s)
                b = e
            return a, b
        if kind == "alt":
            a, b = self.state(), self.state()
            for part in node[1]:
                s, e = self.build(part)
                self.eps[a].append(s)
                self.eps[e].append(b)
            return a, b
        _, inner, lo, hi = node
        a = b = self.state()
        for _ in range(lo):
            s, e = self.build(inner)
            self.eps[b].append(s)
            b = e
        if hi is None:
            s, e = self.build(inner)
            loop = self.state()
            self.eps[b].append(loop)
            self.eps[loop].append(s)
            self.eps[e].append(loop)
            return a, loop
        end = self.state()
        self.eps[b].append(end)
        for _ in range(hi - lo):
            s, e = self.build(inner)
            self.eps[b].append(s)
            b = e
            self.eps[b].append(end)
        return a, end

    def closure(self, states):
        seen, stack = set(states), list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


def _determinise(nfa, start, end, n_labels, name):
    first = nfa.closure([start])
    index, order, delta = {first: 0}, [first], []
    k = 0
    while k < len(order):
        if len(order) > 64 * MAX_STATES:
            raise ValueError(f"pattern {name!r} needs more than {64 * MAX_STATES} states before minimisation: too large")
        row = [-1] * n_labels
        targets = {}
        for s in order[k]:
            for labels, t in nfa.moves[s]:
                for c in labels:
                    targets.setdefault(c, set()).add(t)
        for c, ts in targets.items():
            nxt = nfa.closure(ts)
            if nxt not in index:
                index[nxt] = len(order)
                order.append(nxt)
            row[c] = index[nxt]
        delta.append(row)
        k += 1
    return delta, [end in s for s in order]


def _trim(delta, accept, name):
    n = len(delta)
    back = [[] for _ in range(n)]
    for s, row in enumerate(delta):
        for t in row:
            if t >= 0:
                back[t].append(s)
    live, stack = set(s for s in range(n) if accept[s]), [s for s in range(n) if accept[s]]
    while stack:
        for p in back[stack.pop()]:
            if p not in live:
                live.add(p)
                stack.append(p)
    if 0 not in live:
        raise ValueError(f"pattern {name!r} matches no text over the alphabet: its language is empty")
    keep = sorted(live)
    new = {s: i for i, s in enumerate(keep)}
    return [[new.get(t, -1) for t in delta[s]] for s in keep], [accept[s] for s in keep]


def _minimise(delta, accept):
    cls = [int(a) for a in accept]
    while True:
        sig = {}
        nxt = []
        for s, row in enumerate(delta):
            key = (cls[s], tuple(-1 if t < 0 else cls[t] for t in row))
            nxt.append(sig.setdefault(key, len(sig)))
        if len(sig) == len(set(cls)):
            break
        cls = nxt
    # breadth-first from the start's class, labels ascending
    rep = {}
    for s, c in enumerate(cls):
        rep.setdefault(c, s)
    order, seen, k = [cls[0]], {cls[0]: 0}, 0
    while k < len(order):
        for t in delta[rep[order[k]]]:
            if t >= 0 and cls[t] not in seen:
                seen[cls[t]] = len(order)
                order.append(cls[t])
        k += 1
    out = [[-1 if t < 0 else seen[cls[t]] for t in delta[rep[c]]] for c in order]
    return np.asarray(out, np.int32).reshape(len(order), -1), np.asarray([accept[rep[c]] for c in order], np.uint8)


def label_nodes(delta):
    """How many (state, label entering it) pairs the table has: the label nodes of the decode"""
    delta = np.asarray(delta)
    return len({(int(t), c) for row in delta for c, t in enumerate(row) if t >= 0})


def compile_pattern(name, regex, alphabet, lowercase=False):
    """``(delta (S, len(alphabet)) int32 with -1 for no move, accept (S,) uint8)``: the canonical trimmed minimal automaton
    of ``regex``, start state 0.  ValueError as the module describes; naming the pattern and its count for more than 256
    states or 4096 label nodes, and for an empty language."""
    if not isinstance(regex, str):
        raise ValueError(f"pattern {name!r} must be a string, got {type(regex).__name__}")
    tree = _Parser(name, regex, alphabet, lowercase).parse()
    nfa = _Nfa()
    start, end = nfa.build(tree)
    delta, accept = _minimise(*_trim(*_determinise(nfa, start, end, len(alphabet), name), name))
    if len(delta) > MAX_STATES:
        raise ValueError(f"pattern {name!r} has {len(delta)} states: at most {MAX_STATES} (KOCR_PATTERN_MAX_STATES)")
    nodes = label_nodes(delta)
    if nodes > MAX_NODES:
        raise ValueError(f"pattern {name!r} has {nodes} label nodes: at most {MAX_NODES} (KOCR_PATTERN_MAX_NODES)")
    return delta, accept


class Patterns:
    """``Patterns(alphabet, {"name": regex, ...}, lowercase=False)``: the compiled automata in the mapping's order.
    ``names``; ``delta[i]`` / ``accept[i]``; ``tables()`` for ``Context.set_patterns``.  ValueError for no or more than 64
    patterns, for a name that is not a string and for everything ``compile_pattern`` refuses."""

    def __init__(self, alphabet, patterns, lowercase=False):
        if not hasattr(patterns, "items"):
            raise ValueError(f"patterns must be a mapping name -> regular expression, got {type(patterns).__name__}")
        if not 1 <= len(patterns) <= MAX_PATTERNS:
            raise ValueError(f"{len(patterns)} patterns: there must be between 1 and {MAX_PATTERNS}")
        self.alphabet, self.classes = alphabet, len(alphabet) + 1
        self.names, self.regex, self.delta, self.accept = [], [], [], []
        for i, (name, regex) in enumerate(patterns.items()):
            if not isinstance(name, str):
                raise ValueError(f"pattern {i} has the name {name!r}: names are strings")
            d, a = compile_pattern(name, regex, alphabet, lowercase)
            self.names.append(name)
            self.regex.append(regex)
            self.delta.append(d)
            self.accept.append(a)

    def __len__(self):
        return len(self.names)

    def tables(self):
        """``(delta (sum S, classes - 1) int32, accept (sum S,) uint8, n_states (P,) int32)``"""
        return (np.ascontiguousarray(np.concatenate(self.delta), np.int32), np.ascontiguousarray(np.concatenate(self.accept), np.uint8),
                np.asarray([len(d) for d in self.delta], np.int32))

    def accepts(self, index, labels):
        """Whether pattern ``index`` accepts the label sequence"""
        s = 0
        for c in labels:
            s = int(self.delta[index][s, c])
            if s < 0:
                return False
        return bool(self.accept[index][s])


def index_of(names, pattern):
    """The index of the pattern called ``pattern`` among the loaded ``names`` (None stays None); ValueError listing the loaded
    names for an unknown one."""
    if pattern is None:
        return None
    if not isinstance(pattern, str) or pattern not in (names or []):
        raise ValueError(f"unknown pattern {pattern!r}: the loaded patterns are {list(names or [])} (Recognizer.set_patterns)")
    return names.index(pattern)


def per_box(names, pattern, box_groups):
    """``pattern`` for ``recognize_from_boxes``: None -> (None, None); a name -> (its index, None): one pattern for every box;
    per-image lists of per-box name-or-None -> (None, the flat list of indices, -1 for None).  ValueError for an unknown
    name and for lists that do not match ``box_groups``."""
    if pattern is None or isinstance(pattern, str):
        return index_of(names, pattern), None
    groups = list(pattern)
    if len(groups) != len(box_groups):
        raise ValueError(f"pattern: {len(groups)} per-image lists for {len(box_groups)} box groups")
    flat = []
    for i, (pats, boxes) in enumerate(zip(groups, box_groups)):
        pats = [pats] * len(boxes) if pats is None or isinstance(pats, str) else list(pats)
        if len(pats) != len(boxes):
            raise ValueError(f"pattern: image {i} has {len(pats)} entries for {len(boxes)} boxes")
        flat.extend(-1 if name is None else index_of(names, name) for name in pats)
    return None, np.asarray(flat, np.int32)
