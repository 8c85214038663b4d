"""CPU half of the life-cycle tests (tests/test_lifecycle_gpu.py): what makes the memory accounting of
kocr_debug_memory_stats complete, and the lists of tests/lifecycle_cases.py held against the library's source."""
import os
import re

import numpy as np

from tests import lifecycle_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "keras_ocr_amd", "csrc")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".cpp", ".hip", ".h")))


def _code(name):
    """the file without its // comments (a comment may speak of the runtime's allocator)"""
    text = open(os.path.join(CSRC, name), errors="replace").read()
    return "\n".join(line.split("//", 1)[0] for line in text.splitlines())


def _body(code, signature):
    """the braces' content of the function whose definition starts with ``signature``"""
    at = code.index(signature)
    start = code.index("{", at)
    depth = 0
    for i in range(start, len(code)):
        depth += {"{": 1, "}": -1}.get(code[i], 0)
        if depth == 0:
            return code[start:i + 1], start, i + 1
    raise AssertionError(signature)


def test_the_allocator_is_called_in_the_counted_helpers_only():
    """Every device allocation and every free of the library goes through kocr_counted_malloc / kocr_counted_free (api.cpp):
    the runtime's two calls occur once each, inside them, and nowhere else in csrc -- not in a string either."""
    assert len(SOURCES) > 30
    api = _code("api.cpp")
    malloc_body, m0, m1 = _body(api, "hipError_t kocr_counted_malloc(void** p, size_t bytes)")
    free_body, f0, f1 = _body(api, "hipError_t kocr_counted_free(void* p)")
    assert malloc_body.count("hipMalloc(") == 1 and "hipFree(" not in malloc_body
    assert free_body.count("hipFree(") == 1 and "hipMalloc(" not in free_body
    outside = api[:m0] + api[m1:f0] + api[f1:]
    for name in SOURCES:
        code = outside if name == "api.cpp" else _code(name)
        for call in ("hipMalloc", "hipFree", "hipMallocAsync", "hipFreeAsync", "hipMallocManaged", "hipHostMalloc", "hipExtMallocWithFlags"):
            assert not re.search(rf"\b{call}\s*\(", code), f"{name} calls {call} outside the counted helpers"
    # the counters move with the calls
    assert "g_mem_count += 1" in malloc_body and "g_mem_bytes += bytes" in malloc_body
    assert "g_mem_count -= 1" in free_body and "g_mem_bytes -= " in free_body


def test_the_accounting_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "kocr.h")).read()
    assert re.search(r"int kocr_debug_memory_stats\(kocr_ctx\* ctx, uint64_t\* persistent_count, uint64_t\* persistent_bytes, "
                     r"uint64_t\* arena_bytes,\s*uint64_t\* process_count, uint64_t\* process_bytes\);", header)
    assert '"kocr_debug_memory_stats"' in open(os.path.join(ROOT, "keras_ocr_amd", "_lib.py")).read()
    from tests import workspace_cases as wc
    assert "kocr_debug_memory_stats" in wc.NO_ARENA


def test_the_derived_copies_are_the_release_list():
    """lifecycle_cases.DERIVED_COPIES names every pointer release_layer (conv_mfma.hip) gives back, the layer's own five
    (fp32 weights and the two affines, which every kernel family reads) apart; ConvLayer (common.h) has no device pointer
    that the list misses."""
    body, _, _ = _body(_code("conv_mfma.hip"), "int release_layer(kocr_ctx* ctx, ConvLayer& L)")
    released = set(re.findall(r"L\.(d_[a-z0-9_]+)", body.split("};", 1)[0]))
    own = {"d_w", "d_pre_a", "d_pre_b", "d_post_a", "d_post_b"}
    assert released - own == set(lc.DERIVED_COPIES)
    struct, _, _ = _body(_code("common.h"), "struct ConvLayer")
    assert set(re.findall(r"\*\s*(d_[a-z0-9_]+)\s*=\s*nullptr", struct)) == released
    # every released pointer is cleared behind the release
    for p in released:
        assert re.search(rf"L\.{p} = ", body.split("};", 1)[1]), p
    assert set(lc.DETECTOR_UNREACHED) < set(lc.DERIVED_COPIES)
    assert all(len(reason) > 40 for reason in lc.DETECTOR_UNREACHED.values())


def test_the_lazy_buffers_are_the_ones_the_code_allocates():
    """lifecycle_cases.LAZY_BUFFERS against the code: outside the loaders and the table setters, a context allocates
    persistently in three places only"""
    api = _code("api.cpp")
    assert lc.LAZY_BUFFERS["amax_pool"][0] == 4 * (1 << 16) and "AMAX_SLOTS = 1 << 16" in _code("common.h")
    assert "dev_alloc(&d, AMAX_SLOTS * sizeof(unsigned))" in _body(api, "int kocr_ctx::amax_begin()")[0]
    maps = _body(api, "int kocr_compute_maps(")[0]
    assert "upload(&ctx->d_div255, table)" in maps and lc.LAZY_BUFFERS["div255"][0] == 4 * 256
    assert "dev_alloc(&d, 64)" in _body(api, "int kocr_range_stats_enable(")[0] and lc.LAZY_BUFFERS["range_block"][0] == 64
    assert set(lc.FIRST_CALL_ADDS) == {"amax_pool", "div255"}
    # every other persistent allocation: a loader's (prepare_*, the recurrent kernels, the normalisation table) or a table's
    allowed = {"api.cpp": 7, "crnn.cpp": 1, "craft.cpp": 1, "conv_mfma.hip": 7, "conv_w43.hip": 1, "conv_w43h.hip": 2, "conv_hsplit.hip": 4,
               "conv_wsplit.hip": 1, "conv_dsplit.hip": 1, "conv_k5.hip": 1}
    for name in SOURCES:
        n = len(re.findall(r"ctx->(?:dev_alloc|upload)\(|(?<![>\w])dev_alloc\(&", _code(name)))
        if name == "common.h":
            continue  # the declarations and dev_alloc's own definition
        assert n == allowed.get(name, 0), f"{name}: {n} persistent allocations, {allowed.get(name, 0)} are accounted for"
    # kocr_conv2d_*: the slot pool is there before the temporary layer's mark is taken
    for fn in ("int kocr_conv2d_nhwc(", "int kocr_conv2d_cells("):
        body = _body(api, fn)[0]
        assert 0 < body.index("ctx->amax_begin()") < body.index("TempLayer layer(ctx)")


def test_the_loaders_validate_before_they_change():
    """both loaders call the host-only check (load_check.h, which includes nothing of HIP) before the first line that touches
    the context, and clear `loaded` before the first layer is prepared"""
    check = open(os.path.join(CSRC, "load_check.h")).read()
    assert "hip" not in "\n".join(line for line in check.splitlines() if line.startswith("#include")).lower()
    for name, fn, call, net in (("crnn.cpp", "int crnn_load(", "crnn_check_blobs(", "ctx->crnn = new CrnnNet()"),
                                ("craft.cpp", "int craft_load(", "craft_check_blobs(", "ctx->craft = new CraftNet()")):
        body = _body(_code(name), fn)[0]
        order = [body.index(call), body.index(net), body.index("net->loaded = false"), body.index("prepare_conv("),
                 body.rindex("net->loaded = true")]
        assert order == sorted(order), (name, order)


def test_the_cases_are_what_they_say():
    w, s = lc.crnn_set(seed=5), lc.crnn_set(seed=5, scaled=True)
    assert set(w) == set(s) and len(w) == 50
    for k in w:
        if k.endswith(("/kernel", "/recurrent_kernel", "/bias")):
            ratio = s[k] / np.where(w[k] == 0, 1, w[k])
            want = np.ldexp(np.float32(1), (np.arange(w[k].shape[-1]) % 5) - 2)
            assert np.array_equal(np.broadcast_to(want, w[k].shape)[w[k] != 0], ratio[w[k] != 0]), k
        else:
            assert np.array_equal(w[k], s[k]), k
    c, cs = lc.craft_set(seed=7), lc.craft_set(seed=7, scaled=True)
    assert np.array_equal(cs["basenet.slice1.0.weight"][3], c["basenet.slice1.0.weight"][3] * 2)      # 2^((3 % 5) - 2)
    assert np.array_equal(cs["conv_cls.8.bias"], c["conv_cls.8.bias"] * np.float32([0.25, 0.5]))
    assert np.array_equal(cs["basenet.slice1.1.weight"], c["basenet.slice1.1.weight"])                # BatchNorm stays
    assert not any(k.startswith("stn_") for k in lc.crnn_set(seed=5, stn=False)) and len(lc.crnn_set(seed=5, stn=False)) == 42
    assert lc.crnn_set(seed=5, classes=96)["fc_12/bias"].shape == (96,)
    # every defect removes or resizes exactly the tensor its refusal names
    for defects, make in ((lc.CRNN_DEFECTS, lc.crnn_set), (lc.CRAFT_DEFECTS, lc.craft_set)):
        for name, tensor, what, b, damage in defects:
            good, bad = make(**b), damage(make(**b))
            changed = {k for k in good if k not in bad or bad[k].size != good[k].size}
            assert changed == {tensor}, name
            assert (tensor in bad) == (what == "has wrong size"), name
    delta, accept, n_states = lc.too_many_nodes(37)
    assert delta.shape == (256, 36) and delta.min() >= 0 and delta.max() == 255 and accept.all() and n_states.tolist() == [256]
    assert len({(int(t), c) for row in delta for c, t in enumerate(row)}) == 256 * 36 > 4096  # label nodes: (state entered, class)
