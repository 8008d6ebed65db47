"""conv2 + conv3 of a 32-channel block as two launches vs the wave-specialised fused pair, in the plain, pooled and output-head
forms: equality (bit for bit) and time.  Arguments: tiles (288), tile size (224), and "alias" to use the input as the residual."""
import sys

import torch

sys.path.insert(0, ".")
from aliby_amd import _lib  # noqa: E402
from aliby_amd.extraction.engine import FeatureEngine, _ptr, _stream_ptr  # noqa: E402

eng = FeatureEngine()
N = int(sys.argv[1]) if len(sys.argv) > 1 else 288
H = W = int(sys.argv[2]) if len(sys.argv) > 2 else 224
g = torch.Generator().manual_seed(3)
x = torch.randn(N, H, W, 32, generator=g).to(torch.bfloat16).cuda()
res = torch.randn(N, H, W, 32, generator=g).to(torch.bfloat16).cuda()
if len(sys.argv) > 3 and sys.argv[3] == "alias":  # the network's case: a block's residual is the tensor its first unit reads
    res = x
pk = []
for k in range(2):
    w = (torch.randn(32, 32, 3, 3, generator=g) * 0.06).float().cuda()
    p = torch.empty(32 * 32 * 9, dtype=torch.bfloat16, device="cuda")
    _lib.check(eng.lib.aliby_nn_pack_conv3x3_bf16(eng.ctx.handle, _ptr(w), 32, 32, 32, _ptr(p), _stream_ptr()))
    pk.append(p)
sc = [(torch.rand(32, generator=g) + 0.5).float().cuda() for _ in range(2)]
sh = [(torch.randn(N, 32, generator=g) * 0.2).float().cuda() for _ in range(2)]
bi = [(torch.randn(32, generator=g) * 0.1).float().cuda() for _ in range(2)]
mid = torch.empty_like(x)
out2, out1 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
pool2 = torch.full((N, H // 2, W // 2, 32), float("nan"), dtype=torch.bfloat16, device="cuda")
pool1 = torch.full_like(pool2, float("nan"))
hs, hb = (torch.rand(32, generator=g) + 0.5).float().cuda(), (torch.randn(32, generator=g) * 0.2).float().cuda()
hw, hbias = (torch.randn(3, 32, generator=g) * 0.3).float().cuda(), torch.randn(3, generator=g).float().cuda()
head2, head1 = torch.full((N, 3, H, W), float("nan"), device="cuda"), torch.full((N, 3, H, W), float("nan"), device="cuda")


def two(form):
    pool = form == "pool"
    _lib.check(eng.lib.aliby_nn_conv3x3_bf16(eng.ctx.handle, _ptr(x), _ptr(pk[0]), _ptr(mid), _ptr(sc[0]), _ptr(sh[0]), 32, _ptr(bi[0]), 0, 0,
                                             N, H, W, 32, 32, 0, 0, 0, 0, 0, 0, _stream_ptr()))
    if form == "head":  # the unit with the output head in its epilogue, its own output not written: the network's last two launches
        _lib.check(eng.lib.aliby_nn_conv3x3_head_bf16(eng.ctx.handle, _ptr(mid), _ptr(pk[1]), 0, _ptr(sc[1]), _ptr(sh[1]), 32, _ptr(bi[1]), _ptr(res), 0,
                                                      N, H, W, 32, 32, _ptr(hs), _ptr(hb), _ptr(hw), _ptr(hbias), 3, _ptr(head2), _stream_ptr()))
        return
    _lib.check(eng.lib.aliby_nn_conv3x3_bf16(eng.ctx.handle, _ptr(mid), _ptr(pk[1]), _ptr(out2), _ptr(sc[1]), _ptr(sh[1]), 32, _ptr(bi[1]), _ptr(res), 0,
                                             N, H, W, 32, 32, 0, 0, 0, 0, 0, _ptr(pool2) if pool else 0, _stream_ptr()))


def one(form):
    pool, head = form == "pool", form == "head"
    _lib.check(eng.lib.aliby_nn_conv3x3_pair_bf16(eng.ctx.handle, _ptr(x), _ptr(pk[0]), _ptr(pk[1]), 0 if head else _ptr(out1), _ptr(sc[0]), _ptr(sh[0]), 32,
                                                  _ptr(bi[0]), _ptr(sc[1]), _ptr(sh[1]), 32, _ptr(bi[1]), _ptr(res), N, H, W,
                                                  _ptr(pool1) if pool else 0, _ptr(hs) if head else 0, _ptr(hb) if head else 0,
                                                  _ptr(hw) if head else 0, _ptr(hbias) if head else 0, 3 if head else 0,
                                                  _ptr(head1) if head else 0, _stream_ptr()))


for form in ("plain", "pool", "head"):
    two(form)
    one(form)
    torch.cuda.synchronize()
    equal = torch.equal(head1, head2) if form == "head" else torch.equal(out1, out2) and (form != "pool" or torch.equal(pool1, pool2))
    print(f"{form}: outputs equal: {equal}", flush=True)
    for name, fn in (("two launches", two), ("fused pair", one)):
        for _ in range(3):
            fn(form)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn(form)
        e1.record()
        torch.cuda.synchronize()
        print(f"  {name}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us", flush=True)
