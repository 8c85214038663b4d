"""What the eight decoding recogniser entry points of the C ABI refuse -- kocr_crnn_forward, _forward_scores, _beam, _lexicon,
_pattern, _decode_logits, _decode_logits_charsets, _decode_logits_patterns -- with the code and the literal message of each
refusal, in the order the checks come, and that a call of no crops returns OK and writes nothing.  The messages are those of
the sources before the entry points were put on one staged call; since then the shared body of the two decode_logits entries
names the entry that was called in every message (PREFIX_CHARSETS; before: kocr_crnn_decode_logits in some of them).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, C, LW = 50, 37, 48
PREFIX_CHARSETS = "kocr_crnn_decode_logits_charsets"


def _p(a):
    return None if a is None else a.ctypes.data


class Calls:
    """The eight entries on one context, each with complete and valid arguments for M crops unless told otherwise."""

    def __init__(self, c):
        self.c, self.lib, self.h = c, c._lib, c._h  # pylint: disable=protected-access
        self.crops = np.zeros((2, 31, 200), np.float32)
        self.logits = np.zeros((2, T, C), np.float32)
        self.many = np.zeros(1025, np.int32)
        self.out = {}

    def buf(self, name, shape, dtype):
        self.out[name] = np.full(shape, 77, dtype)
        return self.out[name]

    def args(self, names, over):
        shapes = dict(labels=((2, LW), np.int32), probs=((2, LW, C), np.float32), log_word=((2,), np.float32),
                      char_scores=((2, LW), np.float32), beam_labels=((2, 3, LW), np.int32), beam_log_prob=((2, 3), np.float32),
                      lex_index=((2, 2), np.int32), lex_log_prob=((2, 2), np.float32), lex_values=((2, 3), np.float32),
                      log_path=((2,), np.float32), log_prob=((2,), np.float32))
        self.out = {}
        return [_p(over[n]) if n in over else _p(self.buf(n, *shapes[n])) for n in names]

    def forward(self, M=2, crops="crops", **over):
        return self.lib.kocr_crnn_forward(self.h, _p(getattr(self, crops or "", None)), M, *self.args(["labels", "probs"], over), 0)

    def forward_scores(self, M=2, crops="crops", **over):
        return self.lib.kocr_crnn_forward_scores(self.h, _p(getattr(self, crops or "", None)), M,
                                                 *self.args(["labels", "probs", "log_word", "char_scores"], over), 0)

    def beam(self, M=2, crops="crops", beam_width=4, top_paths=3, **over):
        a = self.args(["beam_labels", "beam_log_prob"], over)
        return self.lib.kocr_crnn_beam(self.h, _p(getattr(self, crops or "", None)), M, beam_width, top_paths, *a, 0)

    def lexicon(self, M=2, crops="crops", top_words=2, **over):
        a = self.args(["lex_index", "lex_log_prob", "lex_values"], over)
        return self.lib.kocr_crnn_lexicon(self.h, _p(getattr(self, crops or "", None)), M, top_words, *a, 0)

    def pattern(self, M=2, crops="crops", pattern_of=None, **over):
        a = self.args(["labels", "log_path", "log_prob"], over)
        return self.lib.kocr_crnn_pattern(self.h, _p(getattr(self, crops or "", None)), M, _p(pattern_of), *a, 0)

    def decode_logits_patterns(self, M=2, logits="logits", pattern_of=None, **over):
        a = self.args(["labels", "log_path", "log_prob"], over)
        return self.lib.kocr_crnn_decode_logits_patterns(self.h, _p(getattr(self, logits or "", None)), M, _p(pattern_of), *a)

    def _decode_logits(self, fn, tail, M, logits, beam_width, top_paths, top_words, over):
        a = self.args(["labels", "probs", "log_word", "char_scores", "beam_labels", "beam_log_prob", "lex_index", "lex_log_prob",
                       "lex_values"], over)
        return fn(self.h, _p(getattr(self, logits or "", None)), M, *a[:4], beam_width, top_paths, *a[4:6], top_words, *a[6:],
                  None, 0, None, None, None, *tail)

    def decode_logits(self, M=2, logits="logits", beam_width=0, top_paths=0, top_words=0, **over):
        return self._decode_logits(self.lib.kocr_crnn_decode_logits, (), M, logits, beam_width, top_paths, top_words, over)

    def decode_logits_charsets(self, M=2, logits="logits", beam_width=0, top_paths=0, top_words=0, set_of=None, **over):
        return self._decode_logits(self.lib.kocr_crnn_decode_logits_charsets, (_p(set_of),), M, logits, beam_width, top_paths,
                                   top_words, over)

    def refused(self, rc, code, message):
        got = self.lib.kocr_last_error(self.h).decode()
        assert (rc, got) == (code, message)

    def untouched(self):
        assert self.out and all((a == 77).all() for a in self.out.values())


ENTRIES = ["forward", "forward_scores", "beam", "lexicon", "pattern", "decode_logits", "decode_logits_charsets", "decode_logits_patterns"]
NAMES = {e: "kocr_crnn_" + e for e in ENTRIES}


@pytest.fixture(scope="module")
def loaded(crnn_weights):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    c.load_crnn(crnn_weights)
    assert c.crnn_classes() == C and c.crnn_label_width() == LW
    yield Calls(c)
    c.close()


def test_no_weights():
    import keras_ocr_amd
    from keras_ocr_amd._lib import KOCR_EINVAL, KOCR_ENOWEIGHTS

    c = keras_ocr_amd.Context(0)
    try:
        k = Calls(c)
        for e in ENTRIES:
            k.refused(getattr(k, e)(), KOCR_ENOWEIGHTS, NAMES[e].replace(NAMES["decode_logits_charsets"], PREFIX_CHARSETS)
                      + ": call kocr_load_crnn first")
        # what comes before the weights: the null buffers everywhere, the ranges of kocr_crnn_beam and kocr_crnn_lexicon
        k.refused(k.forward(labels=None), KOCR_EINVAL, "kocr_crnn_forward: null buffer")
        k.refused(k.beam(beam_width=0), KOCR_EINVAL, "kocr_crnn_beam: beam_width 0 outside [1, 64]")
        k.refused(k.lexicon(top_words=0), KOCR_EINVAL, "kocr_crnn_lexicon: top_words 0 outside [1, 64]")
        k.refused(k.lexicon(top_words=65), KOCR_EINVAL, "kocr_crnn_lexicon: top_words 65 outside [1, 64]")
        k.refused(k.decode_logits(log_word=None), KOCR_EINVAL, "kocr_crnn_decode_logits: log_word and char_scores go together")
        # ... and what comes behind them
        k.refused(k.decode_logits(beam_width=65), KOCR_ENOWEIGHTS, "kocr_crnn_decode_logits: call kocr_load_crnn first")
        k.refused(k.pattern(), KOCR_ENOWEIGHTS, "kocr_crnn_pattern: call kocr_load_crnn first")
    finally:
        c.close()


def test_null_buffers(loaded):
    from keras_ocr_amd._lib import KOCR_EINVAL

    k = loaded
    for e, outs in (("forward", ["labels"]), ("forward_scores", ["labels", "log_word", "char_scores"]),
                    ("beam", ["beam_labels", "beam_log_prob"]), ("lexicon", ["lex_index", "lex_log_prob"]),
                    ("pattern", ["labels", "log_path", "log_prob"]), ("decode_logits_patterns", ["labels", "log_path", "log_prob"])):
        src = "logits" if "logits" in e else "crops"
        for kw in [{src: None}] + [{o: None} for o in outs]:
            k.refused(getattr(k, e)(**kw), KOCR_EINVAL, NAMES[e] + ": null buffer")
        k.refused(getattr(k, e)(M=-1), KOCR_EINVAL, NAMES[e] + ": null buffer")
    for e, name in (("decode_logits", "kocr_crnn_decode_logits"), ("decode_logits_charsets", PREFIX_CHARSETS)):
        call = getattr(k, e)
        k.refused(call(logits=None), KOCR_EINVAL, name + ": null buffer")
        k.refused(call(labels=None), KOCR_EINVAL, name + ": null buffer")
        k.refused(call(log_word=None), KOCR_EINVAL, name + ": log_word and char_scores go together")
        k.refused(call(char_scores=None), KOCR_EINVAL, name + ": log_word and char_scores go together")
        k.refused(call(beam_width=4, top_paths=3, beam_labels=None), KOCR_EINVAL, name + ": null beam buffer")
        k.refused(call(beam_width=4, top_paths=3, beam_log_prob=None), KOCR_EINVAL, name + ": null beam buffer")
    # the optional outputs may be null
    assert k.forward(probs=None) == 0
    assert k.decode_logits(probs=None, log_word=None, char_scores=None) == 0


def test_ranges_and_switches(loaded):
    from keras_ocr_amd._lib import KOCR_EINVAL

    k, c = loaded, loaded.c
    # entry, its name (where the message names the entry it was given), the name in the messages of the shared body
    dl = (("decode_logits", "kocr_crnn_decode_logits", "kocr_crnn_decode_logits"),
          ("decode_logits_charsets", "kocr_crnn_decode_logits_charsets", PREFIX_CHARSETS))
    # the beam: kocr_crnn_beam has no "off"; in the decode_logits entries width 0 is "no beam", whatever top_paths says
    k.refused(k.beam(beam_width=0), KOCR_EINVAL, "kocr_crnn_beam: beam_width 0 outside [1, 64]")
    k.refused(k.beam(beam_width=65), KOCR_EINVAL, "kocr_crnn_beam: beam_width 65 outside [1, 64]")
    k.refused(k.beam(beam_width=4, top_paths=5), KOCR_EINVAL, "kocr_crnn_beam: top_paths 5 outside [1, beam_width = 4]")
    k.refused(k.beam(beam_width=4, top_paths=0), KOCR_EINVAL, "kocr_crnn_beam: top_paths 0 outside [1, beam_width = 4]")
    for e, name, shared in dl:
        call = getattr(k, e)
        assert call(beam_width=0, top_paths=9) == 0
        k.refused(call(beam_width=65, top_paths=3), KOCR_EINVAL, name + ": beam_width 65 outside [1, 64]")
        k.refused(call(beam_width=4, top_paths=5), KOCR_EINVAL, name + ": top_paths 5 outside [1, beam_width = 4]")
        k.refused(call(M=1025), KOCR_EINVAL, shared + ": M 1025 exceeds one recogniser batch of 1024")
    # the lexicon: the range, then that one is loaded
    assert c.lexicon_size() == 0
    k.refused(k.lexicon(top_words=0), KOCR_EINVAL, "kocr_crnn_lexicon: top_words 0 outside [1, 64]")
    k.refused(k.lexicon(top_words=65), KOCR_EINVAL, "kocr_crnn_lexicon: top_words 65 outside [1, 64]")
    k.refused(k.lexicon(), KOCR_EINVAL, "kocr_crnn_lexicon: no lexicon is loaded (kocr_set_lexicon first)")
    for e, name, shared in dl:
        call = getattr(k, e)
        k.refused(call(top_words=65), KOCR_EINVAL, name + ": top_words 65 outside [1, 64]")
        k.refused(call(top_words=-1), KOCR_EINVAL, name + ": top_words -1 outside [1, 64]")
        k.refused(call(top_words=2), KOCR_EINVAL, name + ": no lexicon is loaded (kocr_set_lexicon first)")
    c.set_lexicon(np.array([[1, 2, 3], [4, 5, -1], [6, -1, -1]], np.int32), [3, 2, 1])
    try:
        for e, name, shared in dl:
            call = getattr(k, e)
            k.refused(call(top_words=2, lex_index=None), KOCR_EINVAL, shared + ": null lexicon buffer")
            k.refused(call(top_words=2, lex_log_prob=None), KOCR_EINVAL, shared + ": null lexicon buffer")
            assert call(top_words=2, lex_values=None) == 0 and call(top_words=2, beam_width=4, top_paths=3) == 0
        assert k.lexicon() == 0 and k.lexicon(lex_values=None) == 0
    finally:
        c.set_lexicon(None)
    # the patterns: loaded, one switched on or a list, the list in range, no active character set
    for e in ("pattern", "decode_logits_patterns"):
        k.refused(getattr(k, e)(), KOCR_EINVAL, NAMES[e] + ": no patterns are loaded (kocr_set_patterns first)")
    c.set_patterns(np.zeros((2, C - 1), np.int32), np.ones(2, np.uint8), np.ones(2, np.int32))
    c.set_charsets(np.ones((3, C - 1), np.uint8))
    try:
        for e in ("pattern", "decode_logits_patterns"):
            call = getattr(k, e)
            k.refused(call(), KOCR_EINVAL, NAMES[e] + ": pattern_of is null and no pattern is switched on (kocr_set_pattern)")
            k.refused(call(pattern_of=np.array([0, 2], np.int32)), KOCR_EINVAL,
                      NAMES[e] + ": pattern_of: crop 1 has pattern 2 outside [-1, 2) (2 patterns are loaded: kocr_set_patterns)")
            k.refused(call(pattern_of=np.array([-2, 0], np.int32)), KOCR_EINVAL,
                      NAMES[e] + ": pattern_of: crop 0 has pattern -2 outside [-1, 2) (2 patterns are loaded: kocr_set_patterns)")
            assert call(pattern_of=np.array([-1, 1], np.int32)) == 0
            c.set_charset(1)
            k.refused(call(pattern_of=np.array([0, 1], np.int32)), KOCR_EINVAL,
                      NAMES[e] + ": a pattern cannot be combined with an active character set (kocr_set_charset): the pattern "
                      "states the characters itself")
            c.set_charset(-1)
        k.refused(k.decode_logits_patterns(M=1025, pattern_of=k.many), KOCR_EINVAL,
                  "kocr_crnn_decode_logits_patterns: M 1025 exceeds one recogniser batch of 1024")
        c.set_pattern(1)
        assert k.pattern() == 0 and k.decode_logits_patterns() == 0
        c.set_pattern(-1)
        # the character sets of kocr_crnn_decode_logits_charsets
        k.refused(k.decode_logits_charsets(set_of=np.array([0, 3], np.int32)), KOCR_EINVAL,
                  "kocr_crnn_decode_logits_charsets: set_of: crop 1 has set 3 outside [-1, 3) (3 sets are loaded: kocr_set_charsets)")
        k.refused(k.decode_logits_charsets(set_of=np.array([-2, 0], np.int32)), KOCR_EINVAL,
                  "kocr_crnn_decode_logits_charsets: set_of: crop 0 has set -2 outside [-1, 3) (3 sets are loaded: kocr_set_charsets)")
        assert k.decode_logits_charsets(set_of=np.array([-1, 2], np.int32)) == 0
    finally:
        c.set_pattern(-1)
        c.set_charset(-1)
        c.set_patterns(None)
        c.set_charsets(None)


def test_no_crops(loaded):
    k, c = loaded, loaded.c
    c.set_lexicon(np.array([[1, 2, 3]], np.int32), [3])
    c.set_patterns(np.zeros((1, C - 1), np.int32), np.ones(1, np.uint8), np.ones(1, np.int32))
    c.set_pattern(0)
    try:
        for e in ENTRIES:
            assert getattr(k, e)(M=0) == 0, e
            k.untouched()
        # ... with no buffers at all
        assert k.forward(M=0, crops=None, labels=None, probs=None) == 0
        assert k.beam(M=0, crops=None, beam_labels=None, beam_log_prob=None) == 0
        assert k.decode_logits_patterns(M=0, logits=None, labels=None, log_path=None, log_prob=None) == 0
    finally:
        c.set_pattern(-1)
        c.set_patterns(None)
        c.set_lexicon(None)
