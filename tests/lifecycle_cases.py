"""The cases of tests/test_lifecycle_gpu.py: weight sets, transitions, defects and tables for the moments when a context changes
what it holds ("What a context owns and when it lets go").  Pure numpy on the synthetic weights; nothing
here touches a GPU, and tests/test_lifecycle_cpu.py holds the lists against the library's source.

Every comparison of the GPU tests is bit for bit or of exact integers: a reloaded context must BE a fresh one, a refused load
must change NOTHING.  There is no tolerance in this file or in the tests."""
import functools

import numpy as np

from tests import batch_edge_cases as bc

F32 = np.float32

# the arithmetic modes (set_split_mode): each reads its own derived weight copies.  The first is the default.
MODES = ("f16x2", "bf16x3", "f16x1")

# ---- recogniser batches: one below crnn_small_batch and one at it (tests/test_crnn_layers_gpu.py: 82 | 83 with the default
# switches -- ceil(DSPLIT_MIN_PIXELS / 50)); the per-frame 1x1 layers take another kernel on either side --------------------------
CRNN_BATCHES = (3, 83)


@functools.lru_cache(maxsize=None)
def crops(m):
    x = bc.crops(m)
    x.flags.writeable = False
    return x


# ---- detector pages.  1x32x48 uint8 reads the normalisation table (d_lut) in the first layer's loader, float32 does not; the
# two wider pages are there for the coverage condition alone (DERIVED_COPIES below): 64x96 and 64x512, the page of
# tests/test_craft_layers_gpu.py, whose deeper layers tile exactly (the vertical-reuse F(4,3) kernels) and whose decoder 1x1s
# pass DSPLIT_MIN_PIXELS = 4096 pixels --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def page(h, w, dtype):
    x = np.random.default_rng(1000 * h + w).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    if dtype == "f32":
        x = x.astype(F32) / F32(255) - F32(0.5)
    x.flags.writeable = False
    return x


SMALL_PAGES = ((32, 48, "u8"), (32, 48, "f32"))
COVERAGE_PAGES = ((64, 96, "u8"), (64, 512, "u8"))
DETECTOR_PAGES = SMALL_PAGES + COVERAGE_PAGES


# ---- weight sets ------------------------------------------------------------------------------------------------------------
def _channel_scale(n):
    """2^((c % 5) - 2) per output channel: what made round 4's stale per-channel exponents visible (conv_mfma.hip, prepare_conv)"""
    return np.ldexp(F32(1), (np.arange(n) % 5) - 2).astype(F32)


def scaled_crnn(w):
    """every layer's output channels scaled: the last axis of each kernel and recurrent kernel, and the bias with it"""
    out = {}
    for k, v in w.items():
        if k.endswith(("/kernel", "/recurrent_kernel", "/bias")):
            out[k] = (v * _channel_scale(v.shape[-1])).astype(F32)
        else:
            out[k] = v
    return out


def scaled_craft(w):
    """every convolution's output channels scaled: axis 0 of each OIHW weight, and its bias with it (BatchNorm tensors stay)"""
    out = dict(w)
    for k, v in w.items():
        if k.endswith(".weight") and v.ndim == 4:
            s = _channel_scale(v.shape[0])
            out[k] = (v * s[:, None, None, None]).astype(F32)
            out[k[:-len(".weight")] + ".bias"] = (w[k[:-len(".weight")] + ".bias"] * s).astype(F32)
    return out


@functools.lru_cache(maxsize=None)
def crnn_set(seed=4321, classes=37, stn=True, scaled=False):
    import keras_ocr_amd

    w = dict(keras_ocr_amd.weights.synthetic_crnn_weights(seed, n_classes=classes))
    if scaled:
        w = scaled_crnn(w)
    if not stn:
        w = {k: v for k, v in w.items() if not k.startswith("stn_")}
    return w


@functools.lru_cache(maxsize=None)
def craft_set(seed=1234, scaled=False, calibrated=False):
    import keras_ocr_amd

    w = dict(keras_ocr_amd.weights.synthetic_craft_weights(seed))
    if scaled:
        w = scaled_craft(w)
    if calibrated:  # another last layer, as weights.calibrate_craft_head makes it from a sample of the head's output
        sample = np.random.default_rng(77).normal(0, 1, (1, 16, 24, 2))
        w = keras_ocr_amd.weights.calibrate_craft_head(w, sample, text_frac=0.12, link_frac=0.05)
    return w


# A -> B: (id, crnn_set arguments of A, of B).  B differs from A in everything derived from weights.
CRNN_TRANSITIONS = (
    ("same-twice", dict(seed=4321), dict(seed=4321)),
    ("seed-4321-to-5", dict(seed=4321), dict(seed=5)),
    ("to-scaled", dict(seed=4321), dict(seed=5, scaled=True)),
    ("stn-to-no-stn", dict(seed=4321), dict(seed=5, stn=False)),
    ("no-stn-to-stn", dict(seed=4321, stn=False), dict(seed=5)),
    ("37-to-96-classes", dict(seed=4321), dict(seed=5, classes=96)),
    ("96-to-37-classes", dict(seed=4321, classes=96), dict(seed=5)),
)
# one transition per parametrised case: a detector load folds its linear chain in float64 on the host, the expensive part
CRAFT_TRANSITIONS = (
    ("1234-twice", dict(seed=1234), dict(seed=1234)),
    ("1234-to-7", dict(seed=1234), dict(seed=7)),
    ("to-scaled", dict(seed=1234), dict(seed=7, scaled=True)),
    ("calibrated-to-raw", dict(seed=1234, calibrated=True), dict(seed=1234)),
)

# ---- the coverage condition of the detector half: every derived pointer of release_layer's list (conv_mfma.hip), with the
# profiler rows (a pattern matched at the row's start) of the kernel family that reads it.  The rows of the compared detector
# forwards, over all MODES and DETECTOR_PAGES together, must name a family of each: a stale copy that no compared forward reads
# cannot show. -----------------------------------------------------------------------------------------------------------------
DERIVED_COPIES = {
    "d_ws": r"conv_w[sh]_\d",               # Winograd F(2,3), conv_wsplit.hip
    "d_w4": r"conv_w4[svtnr]?_",             # bf16x3 F(4,3), conv_w43.hip
    "d_w4h": r"conv_w4[hq][vtfr]_",          # fp16 F(4,3), two pieces | one piece, conv_w43h.hip
    "d_ds": r"conv_d[sh]_\d",               # direct convolution, conv_dsplit.hip
    "d_first": r"conv_hs_first_",            # the first layer on raw uint8, conv_hsplit.hip
    "d_hs": r"conv_hs_256x32",               # <= 32 couts, bf16x3
    "d_hs16": r"conv_hs_256x16",             # <= 16 couts
    "d_hsh": r"conv_hh_256x32",              # <= 32 couts, fp16
    "d_pre_a_h": r"conv_hh_256x32|conv_w4[hq][vtfr]_",  # the fp16 kernels' per-cout exponents, undone in pre_a
    "d_k5": r"conv_k5_",                     # 5x5, 16 couts, conv_k5.hip
    "d_w_rgb4": r"conv_mfma_\w+_m2",         # the fp32 MFMA kernel in its uint8 mode, conv_mfma.hip
}
# Copies that no detector page up to 1x64x512 reaches, each with its reason.  None of them is read by the default schedule at
# the benchmark's sizes (detector inputs of 1536 x 1536 and 2048 x 2048).
DETECTOR_UNREACHED = {
    "d_k5": "the 5x5 / 16-cout kernel exists for stn_conv_1 alone: no detector layer has a 5x5 kernel.  The recogniser half of (a) "
            "reads it (the row conv_k5_352x16 is asserted there)",
    "d_w_rgb4": "the uint8 first layer on the fp32 MFMA kernel: taken only when the split first-layer kernel is switched off "
                "(KOCR_FIRST=0) or the image has 2^23 pixels or more (conv_hsplit.hip: first_applicable), twice the benchmark's largest page (2048 x 2048)",
}

# ---- (c) defects: (id, the tensor the refusal names, how B is damaged) --------------------------------------------------------
def _missing(name):
    return lambda w: {k: v for k, v in w.items() if k != name}


def _wrong_size(name):
    return lambda w: dict(w, **{name: np.concatenate([w[name].reshape(-1), np.zeros(1, F32)])})


CRNN_DEFECTS = (
    ("conv_1-kernel-missing", "conv_1/kernel", "missing tensor", dict(seed=5), _missing("conv_1/kernel")),
    ("bn_5-gamma-missing", "bn_5/gamma", "missing tensor", dict(seed=5), _missing("bn_5/gamma")),
    ("lstm_11_back-recurrent-missing", "lstm_11_back/recurrent_kernel", "missing tensor", dict(seed=5),
     _missing("lstm_11_back/recurrent_kernel")),
    ("fc_12-kernel-missing", "fc_12/kernel", "missing tensor", dict(seed=5), _missing("fc_12/kernel")),
    ("conv_4-kernel-wrong-size", "conv_4/kernel", "has wrong size", dict(seed=5), _wrong_size("conv_4/kernel")),
    ("stn_dense_2-bias-missing", "stn_dense_2/bias", "missing tensor", dict(seed=5), _missing("stn_dense_2/bias")),
    ("stn-without-stn_conv_1-kernel", "stn_conv_1/kernel", "missing tensor", dict(seed=5), _missing("stn_conv_1/kernel")),
)
CRAFT_DEFECTS = (
    ("slice1.0-weight-missing", "basenet.slice1.0.weight", "missing tensor", dict(seed=7), _missing("basenet.slice1.0.weight")),
    ("upconv1-running_var-missing", "upconv1.conv.1.running_var", "missing tensor", dict(seed=7), _missing("upconv1.conv.1.running_var")),
    ("conv_cls.8-bias-missing", "conv_cls.8.bias", "missing tensor", dict(seed=7), _missing("conv_cls.8.bias")),
    ("slice3.24-weight-wrong-size", "basenet.slice3.24.weight", "has wrong size", dict(seed=7), _wrong_size("basenet.slice3.24.weight")),
)


# ---- (d) tables ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lexicon(classes, n_words):
    labels, lengths = bc.lexicon(classes, n_words=n_words)
    return labels, lengths


def charsets(classes, n_sets):
    """n_sets sets over the non-blank classes: set s allows every (s + 2)th class"""
    allowed = np.zeros((n_sets, classes - 1), np.uint8)
    for s in range(n_sets):
        allowed[s, ::s + 2] = 1
    return allowed


def patterns(classes, names):
    """(delta, accept, n_states) of the named patterns of tests/pattern_cases.py"""
    from keras_ocr_amd import patterns as kp
    from tests import pattern_cases as pc

    return kp.Patterns(pc.ALPHABETS[classes], {n: pc.PATTERNS[classes][n] for n in names}).tables()


TWO_PATTERNS = {37: ("plate", "digits"), 96: ("short", "digits")}


def too_many_nodes(classes):
    """one trimmed automaton of 256 states that every class enters: 256 (classes - 1) label nodes > KOCR_PATTERN_MAX_NODES = 4096"""
    k = classes - 1
    delta = ((np.arange(256)[:, None] + np.arange(k)[None, :] + 1) % 256).astype(np.int32)
    return delta, np.ones(256, np.uint8), np.array([256], np.int32)


# ---- (e) what the FIRST call of an entry point may add to a context's persistent allocations, taken from the code.  Every item
# is a buffer that is allocated lazily, once, and kept until the context is destroyed: (name, bytes, who allocates it) -------------
LAZY_BUFFERS = {
    "amax_pool": (4 * (1 << 16), "kocr_ctx::amax_begin (api.cpp): the 65536 max-|x| slots of the fp16 kernels' input scales, at "
                                 "the first forward of either network and the first kocr_conv2d_* call"),
    "div255": (4 * 256, "kocr_compute_maps (api.cpp): the float32 table v / 255, at its first call"),
    "range_block": (64, "kocr_range_stats_enable(1) (api.cpp): the counters of one range-statistics launch -- at the switch, "
                        "never inside a call"),
}
# the Context methods whose first call allocates each (the other rows of tests/workspace_cases.py add nothing)
FIRST_CALL_ADDS = {"amax_pool": 1, "div255": 1}
