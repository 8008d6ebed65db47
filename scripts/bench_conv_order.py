"""Does a convolution launch run faster when it walks its tiles against its producer (aliby_nn_conv_order)?  Each
producer -> consumer pair of the network's persistent conv launches runs back to back in this one process at N tiles; the
consumer is timed with device events in the four combinations of (producer, consumer) direction.  "same" = both upwards or both
downwards, "opposite" = the other two.  The combinations are interleaved repetition by repetition, so drift hits all alike.
(run on the GPU box, from the root of the tree whose library is to be timed)
usage: python scripts/bench_conv_order.py [N=288] [repetitions=12]"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from aliby_amd import _lib  # noqa: E402
from aliby_amd.extraction.engine import FeatureEngine, _ptr, _stream_ptr  # noqa: E402

eng = FeatureEngine()
h = eng.ctx.handle
N = int(sys.argv[1]) if len(sys.argv) > 1 else 288
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
ASC, DESC = _lib.CONV_ASCENDING, _lib.CONV_DESCENDING


def bf16(*shape):
    return torch.randn(shape, device="cuda").bfloat16()


class Unit:
    """One convolution unit with random weights: conv3x3(relu(scale * x + shift[n])) + bias (+ res)."""

    def __init__(self, cin, cout, H, in_up=False, entry="aliby_nn_conv3x3_bf16"):
        self.cin, self.cout, self.H, self.in_up, self.entry = cin, cout, H, in_up, entry
        w = torch.randn(cout, cin, 3, 3, device="cuda") / (3 * cin**0.5)
        self.wpk = torch.empty(w.numel(), dtype=torch.bfloat16, device="cuda")
        _lib.check(eng.lib.aliby_nn_pack_conv3x3_bf16(h, _ptr(w), cout, cin, cin, _ptr(self.wpk), _stream_ptr()))
        self.scale = torch.ones(cin, device="cuda")
        self.shift = 0.1 * torch.randn(N, cin, device="cuda")
        self.bias = torch.zeros(cout, device="cuda")

    def __call__(self, x, out, res=None):
        args = [h, _ptr(x), _ptr(self.wpk), _ptr(out), _ptr(self.scale), _ptr(self.shift), 1, _ptr(self.bias), _ptr(res) if res is not None else 0,
                0, N, self.H, self.H, self.cin, self.cout, 1 if self.in_up else 0]
        if self.entry == "aliby_nn_conv3x3_bf16":
            args += [0, 0, 0, 0, 0]
        _lib.check(getattr(eng.lib, self.entry)(*args, _stream_ptr()))


def time_pair(label, producer, consumer):
    """producer() then consumer() REPS times per combination; prints the consumer's time per combination and same against opposite."""
    times = {(p, c): [] for p in (ASC, DESC) for c in (ASC, DESC)}
    for rep in range(REPS + 2):
        for (p, c), ts in times.items():
            _lib.check(eng.lib.aliby_nn_conv_order(h, p))
            producer()
            _lib.check(eng.lib.aliby_nn_conv_order(h, c))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            consumer()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:  # two warm-up rounds
                ts.append(e0.elapsed_time(e1) * 1e3)
    _lib.check(eng.lib.aliby_nn_conv_order(h, _lib.CONV_ALTERNATE))
    name = {ASC: "up", DESC: "down"}
    same = times[(ASC, ASC)] + times[(DESC, DESC)]
    opp = times[(ASC, DESC)] + times[(DESC, ASC)]
    per = "  ".join(f"{name[p]}->{name[c]} {statistics.median(ts):7.1f}" for (p, c), ts in times.items())
    verdict = "opposite median below same minimum" if statistics.median(opp) < min(same) else "no: opposite median not below same minimum"
    print(f"{label} N={N} | us | same median {statistics.median(same):7.1f} [{min(same):7.1f} .. {max(same):7.1f}] | "
          f"opposite median {statistics.median(opp):7.1f} [{min(opp):7.1f} .. {max(opp):7.1f}] | {per} | {verdict}", flush=True)


def chain(label, first, second, x, mid, out, res=None):
    time_pair(label, lambda: first(x, mid), lambda: second(mid, out, res))


a, b = Unit(32, 32, 224), Unit(32, 32, 224)
x, mid, out = bf16(N, 224, 224, 32), bf16(N, 224, 224, 32), bf16(N, 224, 224, 32)
chain("32->32 @224 to 32->32 @224", a, b, x, mid, out)
chain("32->32 @224 to 32->32 @224 + residual", a, b, x, mid, out, res=x)
up = Unit(64, 32, 224, in_up=True)
x64 = bf16(N, 112, 112, 64)
time_pair("64->32 up @224 to 32->32 @224", lambda: up(x64, mid, x), lambda: b(mid, out))
del x, mid, out
a, b = Unit(64, 64, 112), Unit(64, 64, 112)
mid, out = bf16(N, 112, 112, 64), bf16(N, 112, 112, 64)
chain("64->64 @112 to 64->64 @112", a, b, x64, mid, out)
del x64, mid, out
for c, H in ((128, 56), (256, 28)):
    a, b = Unit(c, c, H, entry="aliby_nn_conv3x3_deep_bf16"), Unit(c, c, H, entry="aliby_nn_conv3x3_deep_bf16")
    x, mid, out = bf16(N, H, H, c), bf16(N, H, H, c), bf16(N, H, H, c)
    chain(f"{c}->{c} @{H} to {c}->{c} @{H}", a, b, x, mid, out)
