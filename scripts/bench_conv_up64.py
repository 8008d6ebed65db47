"""Microbenchmark of the up path's 128 -> 64 convolution at 112 x 112 (input through the 2x upsample, skip tensor added): the one
K-loop launch (k_conv3x3_kloop64, csrc/nn_conv_deep.hip) against the two K-slice launches of k_conv3x3 it replaces (run on the
GPU box, from the root of the tree whose library is to be timed).
usage: python scripts/bench_conv_up64.py [kloop|split|both] [N=288]      (split alone touches no symbol older libraries lack)"""
import sys

import torch

sys.path.insert(0, ".")
from aliby_amd import _lib  # noqa: E402
from aliby_amd.extraction.engine import FeatureEngine, _ptr, _stream_ptr  # noqa: E402

eng = FeatureEngine()
what = sys.argv[1] if len(sys.argv) > 1 else "both"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 288
H, cin, cout = 112, 128, 64
x = torch.randn(N, H // 2, H // 2, cin, device="cuda").bfloat16()
w = torch.randn(cout, cin, 3, 3, device="cuda") * 0.05
scale = torch.ones(cin, device="cuda")
shift = torch.zeros(cin, device="cuda")
bias = torch.zeros(cout, device="cuda")
skip = torch.randn(N, H, H, cout, device="cuda").bfloat16()
out = torch.empty(N, H, H, cout, device="cuda", dtype=torch.bfloat16)


def pack(wk):
    pk = torch.empty(wk.numel(), dtype=torch.bfloat16, device="cuda")
    _lib.check(eng.lib.aliby_nn_pack_conv3x3_bf16(eng.ctx.handle, _ptr(wk), cout, wk.shape[1], wk.shape[1], _ptr(pk), _stream_ptr()))
    return pk


wpk, halves = pack(w), [pack(w[:, k0:k0 + 64].contiguous()) for k0 in (0, 64)]
sc2, sh2 = [scale[k0:k0 + 64].contiguous() for k0 in (0, 64)], [shift[k0:k0 + 64].contiguous() for k0 in (0, 64)]


def kloop():
    _lib.check(eng.lib.aliby_nn_conv3x3_kloop64_bf16(eng.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(scale), _ptr(shift), 0, _ptr(bias),
                                                     _ptr(skip), 0, N, H, H, cin, cout, 1, _stream_ptr()))


def split():
    for i, k0 in enumerate((0, 64)):
        _lib.check(eng.lib.aliby_nn_conv3x3_bf16(eng.ctx.handle, _ptr(x), _ptr(halves[i]), _ptr(out), _ptr(sc2[i]), _ptr(sh2[i]), 0,
                                                 _ptr(bias) if i else 0, _ptr(out if i else skip), 0, N, H, H, 64, cout, 1, cin, k0, 0, 0, 0,
                                                 _stream_ptr()))


fl = 2.0 * 9 * cin * cout * N * H * H
byts = 2 * (x.numel() + out.numel() + skip.numel())
for name, run in (("kloop", kloop), ("split", split)):
    if what not in (name, "both"):
        continue
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    label = "one K-loop launch" if name == "kloop" else "two K-slice launches"
    print(f"up64 conv 128->64 up=1 @{H} N={N} {label}: {ms * 1e3:7.1f} us  {fl / ms / 1e9:7.1f} TFLOP/s  {byts / ms / 1e6:7.1f} GB/s alg", flush=True)
