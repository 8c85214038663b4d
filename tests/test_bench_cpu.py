"""CPU suite: the host-side pieces of bench.py (no GPU): synthetic pages, the parity object, the work model behind
the roofline object, and the refusal to report a multi-GPU number from fewer devices."""
import collections
import subprocess
import sys
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pages_are_seeded_and_hold_the_requested_words():
    sys.path.insert(0, ROOT)
    import bench

    a = bench.make_pages(3, 768, seed=4)
    b = bench.make_pages(3, 768, seed=4)
    c = bench.make_pages(3, 768, seed=5)
    assert a.shape == (3, 768, 768, 3) and a.dtype == np.uint8
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # white background with dark glyphs in about WORDS_PER_PAGE grid cells
    dark = (a[0].min(-1) < 128)
    assert 0.002 < dark.mean() < 0.2


def test_parity_object():
    import bench

    box = np.array([[0, 0], [10, 0], [10, 5], [0, 5]], np.float32)
    same = bench.parity_of([("ab", box), ("c", box + 1)], [("ab", box), ("c", box + 1)])
    assert same["ok"] and same["strings_equal"] and same["boxes_max_abs_diff_px"] == 0.0
    moved = bench.parity_of([("ab", box)], [("ab", box + 0.5)])
    assert not moved["ok"] and moved["boxes_max_abs_diff_px"] == 0.5
    text = bench.parity_of([("ab", box)], [("ax", box)])
    assert not text["ok"] and not text["strings_equal"]
    count = bench.parity_of([("ab", box)], [])
    assert not count["ok"] and count["boxes_max_abs_diff_px"] is None
    assert bench.parity_of([], [])["ok"]
    # a box the GPU does not have is accepted only next to a flipped threshold pixel (heat-map px = input px * scale / 2)
    far = bench.parity_of([("ab", box)], [("ab", box), ("c", box + 300)], flipped=np.array([[2, 3]]))
    assert not far["ok"] and far["flip_accounting"]["unexplained"] == 1
    near = bench.parity_of([("ab", box)], [("ab", box), ("c", box + 300)], flipped=np.array([[301, 305]]))
    assert near["ok"] and near["flip_accounting"]["boxes_moved_by_flips"] == 1 and near["flipped_threshold_pixels"] == 1


def test_issued_work_model():
    import keras_ocr_amd as k

    f = k.perfmodel.issued_per_algorithmic
    assert f("conv_w4s_256x128_pool") == {"pipe": "bf16", "factor": 3.0, "why": f("conv_w4s_256x128")["why"]}
    assert f("conv_ws_128x128")["factor"] == 4.0
    assert f("conv_ds_256x128")["factor"] == 6.0 and f("conv_mfma_128x32_m0")["pipe"] == "fp32"
    # round 4: F(4,3) on the fp16 cores -- two pieces / three products (h), one piece / one product (q: fast mode)
    assert f("conv_w4hv_256x128_pool") == {"pipe": "fp16", "factor": 1.5, "why": f("conv_w4ht_256x128")["why"]}
    assert f("conv_w4qv_256x128")["factor"] == 0.5 and f("conv_w4qv_256x128")["pipe"] == "fp16"
    for fam in ("conv_w4v_256x128_pool", "conv_w4t_256x128"):   # round 3: vertical-reuse arrangements
        assert f(fam)["factor"] == 3.0 and f(fam)["pipe"] == "bf16"
    assert f("conv_mfma_128x64_m2")["factor"] == 1.0


def test_bench_refuses_more_ranks_than_gpus():
    """`python bench.py --gpus 2` with fewer than 2 visible GPUs must fail loudly, not print n_gpus: 1."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                       env=env, timeout=600, check=False)
    assert r.returncode != 0
    assert "GPU(s) visible" in (r.stderr + r.stdout)
    assert '"metric"' not in r.stdout


def test_pmc_counter_parsing_and_corrections(tmp_path):
    """keras_ocr_amd.pmc: per-kernel sums over a rocprofv3 counter_collection.csv, the gfx950 FETCH_SIZE correction (KiB,
    doubled) and the profiler-row -> kernel-name mapping bench.py's live traffic measurement relies on."""
    import keras_ocr_amd as k

    d = tmp_path / "fetch"
    d.mkdir()
    rows = ["Dispatch_Id,Kernel_Name,Counter_Name,Counter_Value,Start_Timestamp,End_Timestamp"]
    for i, (name, v) in enumerate([("void conv_w43_kernel<0, 0, 0>(W4Params)", 1000.0), ("void conv_w43_kernel<0, 0, 0>(W4Params)", 3000.0),
                                   ("void conv_w43_kernel<1, 0, 0>(W4Params)", 7.0), ("maxpool2x2_kernel(EwParams)", 512.0)]):
        rows.append(f'{i},"{name}",FETCH_SIZE,{v},{100 * i},{100 * i + 40}')
    (d / "p_counter_collection.csv").write_text("\n".join(rows) + "\n")
    agg, n = k.pmc.load_counters(str(tmp_path))
    kern = k.pmc.find_kernel(agg.keys(), "conv_w4s_256x128")
    assert kern.startswith("void conv_w43_kernel<0, 0, 0") and n[kern] == 2
    assert agg[kern]["FETCH_SIZE"] == 4000.0 and agg[kern]["_ns_FETCH_SIZE"] == 80
    assert k.pmc.fetch_bytes(agg[kern]["FETCH_SIZE"]) / n[kern] == 2000 * 1024 * 2
    assert k.pmc.write_bytes(10.0) == 10240
    assert k.pmc.find_kernel(agg.keys(), "conv_w4s_256x128_pool").startswith("void conv_w43_kernel<1")
    assert k.pmc.find_kernel(agg.keys(), "conv_hs_256x32") is None and k.pmc.find_kernel(agg.keys(), "no_such_row") is None
    assert k.perfmodel.issued_per_algorithmic("conv_hs_256x32")["factor"] == 6.0
    assert abs(k.perfmodel.issued_per_algorithmic("conv_hs_256x16")["factor"] - 60.0 / 9.0) < 1e-12
    assert abs(k.perfmodel.issued_per_algorithmic("conv_k5_352x16:stn_conv_1")["factor"] - 6.24) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# bench.main() executed at WORLD SIZE 2 without a GPU: torch.distributed over gloo, libkocr replaced
# at the ctypes seam by a double (the real Pipeline / Detector / Recognizer / ShardedPipeline classes run), device
# plumbing replaced by bench.GpuEnv's host double.  Checks what a first 8-GPU run would otherwise be the first to
# execute: ONE JSON line from rank 0 only, whole-job accounting (n_gpus, global batch, the sharded batch carries
# world x batch pages on every rank, rank 0 alone sends in the scatter leg), and that no rank sits in a collective while
# rank 0 runs its solo legs (the other rank returns BEFORE rank 0 finishes them).
# ---------------------------------------------------------------------------------------------------------------------
class _BenchMockContext:
    def __init__(self):
        self.mode = 1
        self.prof = False

    def set_split_mode(self, m):
        self.mode = m

    def get_split_mode(self):
        return self.mode

    def profile_reset(self):
        pass

    def profile_enable(self, on=True):
        self.prof = bool(on)

    def profile_report(self):
        return {"conv_w4hv_256x128": {"launches": 6, "ms": 12.0, "flops": 6.0e12, "bytes": 3.0e9},
                "maxpool2x2": {"launches": 2, "ms": 0.5, "flops": 0.0, "bytes": 1.0e9}}

    def load_craft(self, state):
        assert "conv_cls.8.weight" in state

    def load_crnn(self, state):
        assert "fc_12/bias" in state

    def crnn_set_rnn_steps_to_discard(self, steps):
        assert steps == 2

    def crnn_label_width(self):
        return 48

    def resize_pad(self, images, dsize, out_hw=None, cval=255):
        return np.zeros((len(images), 8, 8, 3), np.uint8)

    def craft_forward(self, images, micro_batch=0):
        return np.random.default_rng(0).standard_normal((len(images), 16, 16, 2)).astype(np.float32)

    def get_boxes(self, heat, **kw):
        return [np.zeros((2, 4, 2), np.float32) for _ in range(len(heat))]

    def pipeline(self, images, hs, ws, dhs, dws, hmax, wmax, micro_batch=0, on_device=False, **kw):
        groups, rows = [], []
        for i, (h, dh, dw) in enumerate(zip(hs, dhs, dws)):
            n = 1 + i % 2
            groups.append(np.tile(np.array([[0, 0], [dw, 0], [dw, dh], [0, dh]], np.float32), (n, 1, 1)))
            for j in range(n):
                row = np.full(48, -1, np.int32)
                row[:2] = [int(h) % 36, j]
                rows.append(row)
        return groups, np.array(rows, np.int32)

    def crnn_forward_device(self, d_crops, m, d_labels, d_probs=None):
        import time as _t

        _t.sleep(0.5)   # rank 0's solo legs take a while: the other rank must be gone by then

    def craft_forward_device(self, *a, **kw):
        pass

    def close(self):
        pass


class _HostEnv:
    backend = "gloo"

    def check(self, local_rank):
        pass

    def device_count(self):
        return 2

    def context(self, k, local_rank):
        return _BenchMockContext()

    def sync(self):
        pass

    def to_dev(self, arr):
        import torch

        return torch.from_numpy(np.ascontiguousarray(arr))

    def empty(self, shape, dtype):
        import torch

        return torch.empty(shape, dtype=dtype)

    def rand(self, shape):
        import torch

        return torch.rand(shape)

    def scalar(self, v):
        import torch

        return torch.tensor([v], dtype=torch.float64)

    def cpu_baseline_ok(self):
        return False


def _bench_worker(rank, world, port, q, extra_args=()):
    import time as _t

    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import bench

    res = bench.main(["--gpus", str(world), "--steps", "2", "--warmup", "1", "--batch", "4", "--side5", "64", "--no-live-traffic"]
                     + list(extra_args), env=_HostEnv())
    q.put((rank, _t.time(), res))


def test_bench_main_runs_at_world_2_over_gloo_with_a_mocked_library(capfd):
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bench_worker, args=(r, 2, port, q, ("--full",))) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, t0, res), (_, t1, none) = got
    assert none is None and isinstance(res, dict)                      # one result, from rank 0
    assert t1 < t0 - 1.0                                               # rank 1 left before rank 0's solo legs were over
    assert res["n_gpus"] == 2 and res["ranks_seen"] == 2 and res["steps"] == 2 and res["warmup"] == 1
    assert res["config"]["global_batch"] == 8 and res["scaling"] == "weak" and res["higher_is_better"] is True
    assert abs(res["value"] - 8 * 2 / (res["ms_per_step"] * 2 / 1e3)) < 1e-6 * res["value"]   # whole job: world x batch x K / time
    sh, sc = res["cfg5_sharded"], res["cfg5_scattered"]
    assert sh["pages_returned_on_every_rank"] == 8 and sh["backend"] == "gloo" and sh["gather_ms"] > 0
    assert sc["scatter_bytes_sent_by_rank0"] == 4 * 64 * 64 * 3 and sc["scatter_ms"] > 0 and sc["same_strings_as_resident_blocks"]
    assert res["roofline"]["kernel"] == "conv_w4hv_256x128" and res["roofline"]["peak"] == 2500.0
    assert abs(res["roofline"]["issued_tflops"] - 1.5 * res["roofline"]["achieved"]) < 1e-9
    assert "cpu_baseline" not in res and res["crnn_only"]["value"] > 0
    out = capfd.readouterr().out
    assert sum(ln.startswith('{"metric"') for ln in out.splitlines()) == 1   # exactly one JSON line on stdout


class _CountingMockContext(_BenchMockContext):
    """The library double, counting the calls of a run that go beyond setting up."""

    def __init__(self):
        super().__init__()
        self.calls = collections.Counter()

    def pipeline(self, *a, **kw):
        self.calls["pipeline"] += 1
        return super().pipeline(*a, **kw)

    def profile_enable(self, on=True):
        self.calls["profile_enable(True)"] += bool(on)
        super().profile_enable(on)

    def crnn_forward_device(self, *a, **kw):
        self.calls["crnn_forward_device"] += 1

    def craft_forward_device(self, *a, **kw):
        self.calls["craft_forward_device"] += 1


class _CountingHostEnv(_HostEnv):
    def context(self, k, local_rank):
        self.ctx = _CountingMockContext()
        return self.ctx


def _plain_bench_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import bench

    env = _CountingHostEnv()
    res = bench.main(["--gpus", str(world), "--steps", "2", "--warmup", "1", "--batch", "4"], env=env)
    q.put((rank, res, +env.ctx.calls))


def test_bench_plain_run_does_only_the_headline(capfd):
    """Without --full, bench.main() at world size 2 runs the warm-up and the timed steps and nothing else (no profiled loop,
    no extra leg, no solo leg of rank 0), and rank 0 prints the headline keys alone on its one stdout line."""
    import json
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_plain_bench_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, res, calls0), (_, none, calls1) = got
    assert none is None and isinstance(res, dict)
    assert calls0 == calls1 == {"pipeline": 3}                        # 1 warm-up + 2 timed steps per rank
    assert sorted(res) == sorted(["metric", "value", "unit", "n_gpus", "ranks_seen", "steps", "warmup", "ms_per_step",
                                  "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"])
    assert res["n_gpus"] == 2 and res["ranks_seen"] == 2 and res["steps"] == 2 and res["warmup"] == 1
    assert res["config"]["global_batch"] == 8 and res["higher_is_better"] is True and res["unit"] == "images/s"
    assert abs(res["value"] - 8 * 2 / (res["ms_per_step"] * 2 / 1e3)) < 1e-6 * res["value"]
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1 and json.loads(lines[0]) == res


def test_bench_refuses_full_only_options_on_a_plain_run():
    sys.path.insert(0, ROOT)
    import bench

    for opt in ("--alt-mode", "--profile-all"):
        with pytest.raises(SystemExit):
            bench.main([opt], env=_HostEnv())


@pytest.mark.parametrize("pages,blocks", [(14, [4, 4, 4, 2]), (5, [2, 2, 1, 0])], ids=["ragged_last_block", "an_empty_rank"])
def test_bench_main_at_world_4_with_uneven_shards(pages, blocks, capfd):
    """the sharded / scattered legs of bench.main() at world size 4 when the ONE batch does not divide
    evenly -- a short last block, and a rank that gets nothing at all (it must still take part in every collective and end
    with the whole result).  `--cfg5-pages` sets the total; blocks are ceil(n / N) contiguous pages (dist.shard_bounds)."""
    import socket
    import torch.multiprocessing as mp
    import keras_ocr_amd

    assert [e - s_ for s_, e in (keras_ocr_amd.dist.shard_bounds(pages, 4, r) for r in range(4))] == blocks
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bench_worker, args=(r, 4, port, q, ("--full", "--cfg5-pages", str(pages)))) for r in range(4)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res = got[0][2]
    assert all(g[2] is None for g in got[1:]) and isinstance(res, dict)
    assert res["n_gpus"] == 4 and res["ranks_seen"] == 4 and res["config"]["global_batch"] == 16
    sh, sc = res["cfg5_sharded"], res["cfg5_scattered"]
    assert sh["pages_returned_on_every_rank"] == pages                       # every page, on every rank, whatever its block was
    per = -(-pages // 4)
    assert sc["scatter_bytes_sent_by_rank0"] == per * 3 * 64 * 64 * 3        # equal (zero-padded) blocks to the three peers
    assert sc["same_strings_as_resident_blocks"]
    assert abs(sh["value"] - pages * 2 / (sh["ms_per_batch"] * 2 / 1e3)) < 1e-6 * sh["value"]
    out = capfd.readouterr().out
    assert sum(ln.startswith('{"metric"') for ln in out.splitlines()) == 1


@pytest.mark.parametrize("pages,blocks", [(256, [32] * 8), (250, [32] * 7 + [26])], ids=["cfg5_256_pages_equal_blocks", "250_pages_ragged"])
def test_bench_main_at_world_8_the_cfg5_job_shape(pages, blocks, capfd):
    """VERDICT r05 item 7 / SURVEY 8(e): bench.main() at WORLD SIZE 8 over gloo with the job shape of BASELINE configs[4] --
    ONE batch of 256 pages (tiny ones here), 32 per rank -- and the same with 250 pages (a short last block).  Checks the
    N = 8 line's schema: every rank was seen by the all-reduce, every rank ends with all pages, rank 0 sends 7/8 of the
    batch in the scatter leg (equal, zero-padded blocks), whole-job accounting of `value`.  No scaling number is claimed."""
    import socket
    import torch.multiprocessing as mp
    import keras_ocr_amd

    assert [e - s_ for s_, e in (keras_ocr_amd.dist.shard_bounds(pages, 8, r) for r in range(8))] == blocks
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    extra = ("--full", "--cfg5-pages", str(pages), "--batch", "32", "--side5", "16")
    procs = [ctx.Process(target=_bench_worker, args=(r, 8, port, q, extra)) for r in range(8)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=600) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res = got[0][2]
    assert all(g[2] is None for g in got[1:]) and isinstance(res, dict)            # ONE result, from rank 0
    assert res["n_gpus"] == 8 and res["ranks_seen"] == 8 and res["config"]["global_batch"] == 256 and res["scaling"] == "weak"
    assert abs(res["value"] - 256 * 2 / (res["ms_per_step"] * 2 / 1e3)) < 1e-6 * res["value"]
    sh, sc = res["cfg5_sharded"], res["cfg5_scattered"]
    assert sh["pages_returned_on_every_rank"] == pages and sh["backend"] == "gloo" and sh["gather_ms"] > 0
    assert sc["scatter_bytes_sent_by_rank0"] == 32 * 7 * 16 * 16 * 3                # 7/8 of the (padded) batch leave rank 0
    assert sc["same_strings_as_resident_blocks"]
    assert abs(sh["value"] - pages * 2 / (sh["ms_per_batch"] * 2 / 1e3)) < 1e-6 * sh["value"]
    out = capfd.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1                                                          # exactly one JSON line on stdout
    import json

    line = json.loads(lines[0])
    assert line["n_gpus"] == 8 and line["ranks_seen"] == 8 and "crnn_ms_per_crop" in line["config"]
    assert line["legs_images_per_s"]["cfg5_sharded"] > 0 and len(lines[0]) < 6000   # the driver's record holds it whole


def test_bench_dump_outputs_holds_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the headline path's result of its last timed step as .npy arrays (float32 / float64), here from
    the mocked library at world size 1: one box per page, then two, alternately; every word's text as code points."""
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_bench_worker, args=(0, 1, port, q, ("--no-extra", "--dump-outputs", str(tmp_path / "out"))))
    p.start()
    _, _, res = q.get(timeout=300)
    p.join(timeout=60)
    assert p.exitcode == 0 and res["steps"] == 2
    got = {f.stem: np.load(f) for f in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["boxes", "text_codepoints", "words_per_page"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["words_per_page"].tolist() == [1, 2, 1, 2]
    boxes, codes = got["boxes"], got["text_codepoints"]
    assert boxes.shape == (6, 4, 2) and len(codes) == 6
    # the mock's box spans the detector input; back in input pixels it spans the 768 x 768 page
    assert np.array_equal(boxes[0], np.array([[0, 0], [768, 0], [768, 768], [0, 768]], boxes.dtype))
    texts = ["".join(chr(int(c)) for c in row if c >= 0) for row in codes]
    assert all(1 <= len(t) <= 2 for t in texts)


def test_bench_refuses_zero_steps():
    sys.path.insert(0, ROOT)
    import bench

    with pytest.raises(SystemExit):
        bench.main(["--steps", "0"], env=_HostEnv())
