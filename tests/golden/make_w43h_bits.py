"""Generate tests/golden/w43h_bits.json: SHA-256 digests of what the fp16 F(4,3) kernels write (outputs and per-image
max-|x| slots) for the cases of tests/w43h_bits_cases.py.

Run on an MI355X with the library build whose bits are to be kept (the file in the repository was written by the build
BEFORE the input transform of csrc/conv_w43h.hip was rewritten per component):

    python tests/golden/make_w43h_bits.py [output.json]

tests/test_w43h_bits_gpu.py recomputes the digests with the library under test and compares.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import keras_ocr_amd  # noqa: E402
from tests import w43h_bits_cases as wb  # noqa: E402


def main():
    dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "w43h_bits.json")
    ctx = keras_ocr_amd.Context(0)
    try:
        got = wb.digests(ctx, keras_ocr_amd.weights.synthetic_craft_weights(1234), keras_ocr_amd.weights.synthetic_crnn_weights(4321))
    finally:
        ctx.close()
    with open(dest, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{dest}: {len(got['single'])} + {len(got['single_f16x1'])} single layers, "
          f"{sum(len(v) for v in got['craft'].values())} CRAFT taps, {sum(len(v) for v in got['crnn'].values())} recogniser taps")


if __name__ == "__main__":
    main()
