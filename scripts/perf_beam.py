"""Developer probe: what the beam search costs.  Run under `rocprofv3 --kernel-trace --stats`:
  perf_beam.py run B         N rounds of kocr_crnn_forward, kocr_crnn_forward_scores and kocr_crnn_beam(B, top_paths 3) on 512
                             device-resident crops, so that ctc_beam_kernel, ctc_scores_kernel and the forward's kernels come
                             from one run;
  perf_beam.py report B CSV  one line from that run's kernel statistics: the whole forward = every kernel but the two
                             decoders' and the beam, per call, plus ctc_kernel."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M, N, K = 512, 10, 3


def run(beam_width):
    import torch
    import keras_ocr_amd as k

    ctx = k.Context(0)
    ctx.load_crnn(k.weights.synthetic_crnn_weights(4321))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    crops = torch.rand((M, 31, 200), dtype=torch.float32, device="cuda")
    labels = torch.empty((M, 48), dtype=torch.int32, device="cuda")
    logw = torch.empty((M,), dtype=torch.float32, device="cuda")
    chars = torch.empty((M, 48), dtype=torch.float32, device="cuda")
    beam_labels = torch.empty((M, K, 48), dtype=torch.int32, device="cuda")
    beam_logp = torch.empty((M, K), dtype=torch.float32, device="cuda")
    for _ in range(N + 2):  # the first two rounds warm up; they are part of the averages all the same
        ctx.crnn_forward_device(crops.data_ptr(), M, labels.data_ptr())
        ctx.crnn_forward_scores_device(crops.data_ptr(), M, labels.data_ptr(), logw.data_ptr(), chars.data_ptr())
        ctx.crnn_beam_device(crops.data_ptr(), M, beam_width, K, beam_labels.data_ptr(), beam_logp.data_ptr())
    torch.cuda.synchronize()
    ctx.close()


def report(beam_width, path):
    rows = list(csv.DictReader(open(path)))
    tail = {"ctc_kernel": None, "ctc_scores_kernel": None, "ctc_beam_kernel": None}
    rest_ns, calls = 0.0, 0
    for r in rows:
        name = r["Name"]
        key = next((k for k in tail if name.startswith(k) or ("_Z" in name and k in name)), None)
        if key:
            tail[key] = (int(r["Calls"]), float(r["TotalDurationNs"]))
        else:
            rest_ns += float(r["TotalDurationNs"])
    calls = tail["ctc_kernel"][0]
    avg = {k: v[1] / v[0] / 1e3 for k, v in tail.items()}
    forward = rest_ns / (3 * calls) / 1e3 + avg["ctc_kernel"]
    print(f"M {M}  beam_width {beam_width:2d}  top_paths {K}: ctc_beam_kernel {avg['ctc_beam_kernel']:9.1f} us  "
          f"ctc_scores_kernel {avg['ctc_scores_kernel']:7.1f} us  ctc_kernel {avg['ctc_kernel']:6.1f} us  "
          f"whole forward {forward:9.1f} us ({forward / M:.2f} us per crop)  beam / forward {avg['ctc_beam_kernel'] / forward:.3f}  "
          f"[{calls} calls each]")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]))
    else:
        report(int(sys.argv[2]), sys.argv[3])
