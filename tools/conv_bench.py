"""Time the 3x3 convolutions on the Cnn14 layer shapes (random data): python tools/conv_bench.py [batch] [samples]
-> TFLOP/s per layer of the tile conv3x3_bf16 plans for it (gemm_bf16.hip, conv_plan)."""
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from wise_amd import _lib  # noqa: E402
from wise_amd.feature.cnn14 import CHANNELS, HOP  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 480000
lib = _lib.lib()
g = torch.Generator(device="cuda").manual_seed(0)
zeros = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
T, F, cin = N // HOP + 1, 64, 1
for i, cout in enumerate(CHANNELS):
    for j, ci in enumerate((cin, cout)):
        POOL = 1 if (j == 1 and i < len(CHANNELS) - 1) else 0   # the block's second convolution carries the pooling
        if ci >= 64:
            M = B * T * F
            rows = (M + 255) // 256 * 256
            x = torch.randn(rows, ci, generator=g, device="cuda").to(torch.bfloat16)
            w = (torch.randn(cout, 9 * ci, generator=g, device="cuda") * (2.0 / (9 * ci)) ** 0.5).to(torch.bfloat16)
            bias = 0.1 * torch.randn(cout, generator=g, device="cuda")
            out = torch.empty(rows, cout, dtype=torch.bfloat16, device="cuda")
            _lib.check(lib.wise_conv3x3_relu_bf16(x.data_ptr(), w.data_ptr(), bias.data_ptr(), zeros.data_ptr(), B, T, F, ci,
                                                  cout, POOL, out.data_ptr(), _lib.stream_ptr()), "conv")
            torch.cuda.synchronize()
            res = []
            for rnd in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    lib.wise_conv3x3_relu_bf16(x.data_ptr(), w.data_ptr(), bias.data_ptr(), zeros.data_ptr(), B, T, F, ci, cout,
                                               POOL, out.data_ptr(), _lib.stream_ptr())
                e1.record()
                torch.cuda.synchronize()
                res.append(e0.elapsed_time(e1) / 5 * 1e-3)
            fl = 2.0 * (B * (T // 2) * (F // 2) * 4 if POOL else M) * cout * 9 * ci
            t = sorted(res)[1]
            print(f"block {i + 1} conv {j + 1}: M={M:9d} T={T:4d} F={F:2d} {ci:4d}->{cout:4d} | {fl / t / 1e12:6.1f} TF {t * 1e6:7.1f} us",
                  flush=True)
            del x, w, out
    if i < len(CHANNELS) - 1:
        T, F = T // 2, F // 2
    cin = cout
