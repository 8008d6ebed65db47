"""
The up path's 128 -> 64 convolution (input read through the 2x upsample, skip tensor added) as ONE K-loop launch:
aliby_nn_conv3x3_kloop64_bf16 / k_conv3x3_kloop64 (aliby_amd/csrc/nn_conv_deep.hip), which replaces two K-slice launches of
aliby_nn_conv3x3_bf16 with a bf16 partial sum in HBM between them.

  * integer data, where every product and sum is exact: the launch equals a float64 reference bit for bit, for batches of
    1, 2, 9 and 288 images at 112 x 112, at the smallest and at non-square sizes, with and without the skip residual, with a
    shared and with a per-sample shift;
  * random data: its error against a float64 convolution is no larger than the two K-slice launches' error on the same inputs
    (both are computed here, so there is no tolerance constant);
  * image k of a batch of 288 has the bits of the same image launched alone;
  * shapes outside the family are refused with the library's unsupported-shape error, and nothing is launched.
"""

import pytest

pytestmark = pytest.mark.gpu

CIN, COUT = 128, 64


def _ref64(x, w, scale, shift, bias, res, chunk=16):
    """float64 conv3x3(relu(scale * up2(x) + shift) rounded to bf16) + bias + res, NHWC, as nine shifted channel contractions."""
    import torch
    import torch.nn.functional as F

    n, ih, iw, cin = x.shape
    H, W = 2 * ih, 2 * iw
    w64 = w.bfloat16().double()
    out = torch.empty((n, H, W, w.shape[0]), dtype=torch.float64, device=x.device)
    for i0 in range(0, n, chunk):
        sh = shift[i0:i0 + chunk, None, None, :] if shift.ndim == 2 else shift
        # the kernel's prologue is one fp32 fma, then a rounding to bf16
        a = torch.relu(x[i0:i0 + chunk].double() * scale.double() + sh.double()).float().bfloat16().double()
        a = a.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        a = F.pad(a, (0, 0, 1, 1, 1, 1))
        y = torch.zeros((a.shape[0], H, W, w.shape[0]), dtype=torch.float64, device=x.device)
        for dy in range(3):
            for dx in range(3):
                y += a[:, dy:dy + H, dx:dx + W, :] @ w64[:, :, dy, dx].t()
        if bias is not None:
            y += bias.double()
        if res is not None:
            y += res[i0:i0 + chunk].double()
        out[i0:i0 + chunk] = y
    return out


def _pack(engine, w):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    cout, cin = w.shape[0], w.shape[1]
    wpk = torch.empty(cout * cin * 9, dtype=torch.bfloat16, device="cuda")
    _lib.check(engine.lib.aliby_nn_pack_conv3x3_bf16(engine.ctx.handle, _ptr(w.contiguous()), cout, cin, cin, _ptr(wpk), _stream_ptr()))
    return wpk


def _run_kloop64(engine, x, w, scale, shift, bias, res):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, ih, iw, cin = x.shape
    H, W, cout = 2 * ih, 2 * iw, w.shape[0]
    wpk = _pack(engine, w)
    out = torch.full((n, H, W, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    _lib.check(engine.lib.aliby_nn_conv3x3_kloop64_bf16(
        engine.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(scale), _ptr(shift), 1 if shift.ndim == 2 else 0,
        _ptr(bias) if bias is not None else 0, _ptr(res) if res is not None else 0, 0, n, H, W, cin, cout, 1, _stream_ptr()))
    torch.cuda.synchronize()
    return out


def _run_k_split(engine, x, w, scale, shift, bias, res):
    """The two launches the K-loop launch replaces (FusedUNet._unit's K split): input channels 0-63, then 64-127 adding to the
    first launch's bf16 output; the bias rides in the last one."""
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, ih, iw, cin = x.shape
    H, W, cout = 2 * ih, 2 * iw, w.shape[0]
    out = torch.full((n, H, W, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    cur = res
    for k0 in range(0, cin, 64):
        last = k0 + 64 == cin
        wpk = _pack(engine, w[:, k0:k0 + 64].contiguous())
        sh = shift[..., k0:k0 + 64].contiguous()
        _lib.check(engine.lib.aliby_nn_conv3x3_bf16(
            engine.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(scale[k0:k0 + 64].contiguous()), _ptr(sh), 1 if sh.ndim == 2 else 0,
            _ptr(bias) if bias is not None and last else 0, _ptr(cur) if cur is not None else 0, 0, n, H, W, 64, cout, 1, cin, k0, 0, 0, 0,
            _stream_ptr()))
        cur = out
    torch.cuda.synchronize()
    return out


def _integer_case(n, H, W, seed, per_sample_shift):
    import torch

    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 3, (n, H // 2, W // 2, CIN), generator=g).to(torch.bfloat16).cuda()
    w = (torch.randint(-1, 2, (COUT, CIN, 3, 3), generator=g) * (torch.rand(COUT, CIN, 3, 3, generator=g) < 0.05)).float().cuda()
    scale = torch.randint(1, 3, (CIN,), generator=g).float().cuda()
    shift = torch.randint(-1, 2, (n, CIN) if per_sample_shift else (CIN,), generator=g).float().cuda()
    bias = torch.randint(-2, 3, (COUT,), generator=g).float().cuda()
    res = torch.randint(-3, 4, (n, H, W, COUT), generator=g).to(torch.bfloat16).cuda()
    return x, w, scale, shift, bias, res


# 112 x 112 at the batch sizes of the network's use; the smallest map (one pixel in); non-square maps narrower and wider than a
# tile's 448 positions, the widest the kernel takes; a batch that ends inside a tile.  Per-sample shifts where an image holds a
# whole tile window (the entry point refuses them on smaller images), the shared shift of the network's conv0 everywhere
EXACT = [(1, 112, 112, True), (2, 112, 112, True), (9, 112, 112, True), (288, 112, 112, True), (288, 112, 112, False),
         (1, 2, 2, False), (3, 2, 2, False), (5, 8, 8, False), (7, 12, 20, False), (2, 88, 104, True), (3, 56, 72, True),
         (2, 128, 128, True), (5, 32, 48, False), (3, 16, 128, False)]


@pytest.mark.parametrize("n,H,W,per_sample", EXACT)
def test_kloop64_exact_on_integer_data(engine, n, H, W, per_sample):
    import torch

    x, w, scale, shift, bias, res = _integer_case(n, H, W, 1000 * n + 10 * H + W, per_sample)
    ref = _ref64(x, w, scale, shift, bias, res)
    assert float(ref.abs().max()) <= 256  # exactly representable in bf16
    out = _run_kloop64(engine, x, w, scale, shift, bias, res)
    assert torch.equal(out.double(), ref), float((out.double() - ref).abs().max())
    # without the skip residual, without the bias
    out2 = _run_kloop64(engine, x, w, scale, shift, None, None)
    ref2 = _ref64(x, w, scale, shift, None, None)
    assert torch.equal(out2.double(), ref2), float((out2.double() - ref2).abs().max())


def _random_case(n, H, W, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, H // 2, W // 2, CIN), generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn((COUT, CIN, 3, 3), generator=g) / (3 * CIN**0.5)).float().cuda()
    scale = (1 + 0.1 * torch.randn(CIN, generator=g)).float().cuda()
    shift = (0.1 * torch.randn(CIN, generator=g)).float().cuda()
    bias = torch.randn(COUT, generator=g).float().cuda()
    res = torch.randn((n, H, W, COUT), generator=g).to(torch.bfloat16).cuda()
    return x, w, scale, shift, bias, res


def test_kloop64_random_data_is_no_further_from_fp64_than_the_k_split_launches(engine):
    """One bf16 rounding (of the result) against two (the partial sum after 64 channels, then the result)."""
    x, w, scale, shift, bias, res = _random_case(4, 112, 112, 5)
    ref = _ref64(x, w, scale, shift, bias, res)
    one = _run_kloop64(engine, x, w, scale, shift, bias, res).double()
    two = _run_k_split(engine, x, w, scale, shift, bias, res).double()
    err_one = float((one - ref).norm() / ref.norm())
    err_two = float((two - ref).norm() / ref.norm())
    max_one, max_two = float((one - ref).abs().max()), float((two - ref).abs().max())
    print(f"rel-L2 vs float64 reference: K-loop {err_one:.3e} (max abs {max_one:.3e}), K-split launches {err_two:.3e} (max abs {max_two:.3e})")
    assert err_one <= err_two, (err_one, err_two)


def test_kloop64_image_in_a_batch_of_288_has_the_bits_of_the_image_alone(engine):
    import torch

    n = 288
    x, w, scale, shift, bias, res = _random_case(n, 112, 112, 6)
    g = torch.Generator().manual_seed(7)
    shift_n = (0.1 * torch.randn((n, CIN), generator=g)).float().cuda()  # per sample, as the styled units' shifts
    for sh in (shift, shift_n):
        batch = _run_kloop64(engine, x, w, scale, sh, bias, res)
        assert bool(torch.isfinite(batch.float()).all())
        for k in (0, 1, 143, 286, 287):
            sk = sh[k:k + 1].contiguous() if sh.ndim == 2 else sh
            alone = _run_kloop64(engine, x[k:k + 1].contiguous(), w, scale, sk, bias, res[k:k + 1].contiguous())
            assert torch.equal(alone[0], batch[k]), (k, sh.ndim)


@pytest.mark.parametrize("n,H,W,cin,cout,in_up,per_sample", [
    (2, 112, 112, 128, 128, 1, 0),  # the deep kernel's family
    (2, 112, 112, 64, 64, 1, 0),    # k_conv3x3's
    (2, 112, 112, 256, 64, 1, 0),
    (2, 112, 112, 128, 64, 0, 0),   # not through the upsample
    (2, 112, 130, 128, 64, 1, 0),   # wider than the LDS window is sized for
    (2, 224, 224, 128, 64, 1, 0),
    (2, 8, 8, 128, 64, 1, 1),       # per-sample shift on images smaller than a tile window
])
def test_kloop64_refuses_other_shapes_and_launches_nothing(engine, n, H, W, cin, cout, in_up, per_sample):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    ih, iw = (H // 2, W // 2) if in_up else (H, W)
    x = torch.zeros((n, ih, iw, cin), dtype=torch.bfloat16, device="cuda")
    wpk = torch.zeros(cout * cin * 9, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros((n, cin), device="cuda")
    out = torch.full((n, H, W, cout), 7.0, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(Exception, match="unsupported"):
        _lib.check(engine.lib.aliby_nn_conv3x3_kloop64_bf16(
            engine.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(f), _ptr(f), per_sample, 0, 0, 0, n, H, W, cin, cout, in_up, _stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing ran


def test_fused_unet_runs_the_up_block_conv0_as_one_kloop64_launch(engine, monkeypatch):
    """FusedUNet._unit sends (128, 64, upsampled) to the K-loop launch by the shape alone, whatever the batch; with the A/B switch
    off it makes the two K-slice launches."""
    import torch
    from aliby_amd.segment.fused_unet import FusedUNet
    from aliby_amd.segment.unet import build_network

    net = build_network(seed=5, device="cuda")
    fused = FusedUNet(net, engine)
    calls = []
    orig_k, orig_u = FusedUNet._launch_kloop64, FusedUNet._launch_unit
    monkeypatch.setattr(FusedUNet, "_launch_kloop64", lambda s, *a, **k: (calls.append("kloop64"), orig_k(s, *a, **k))[1])
    monkeypatch.setattr(FusedUNet, "_launch_unit", lambda s, *a, **k: (calls.append(("unit", a[2], a[3])), orig_u(s, *a, **k))[1])
    u0 = fused.up[1]["u"][0]
    for n in (1, 9):
        x = torch.randn((n, 128, 56, 56), device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
        skip = torch.randn((n, 64, 112, 112), device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
        calls.clear()
        one = fused._unit(x, u0, bias=u0.bias, res=skip, in_up=True)
        assert calls == [("unit", (0, 128), (0, 64)), "kloop64"], calls
        calls.clear()
        fused.kloop64_kernel = False
        two = fused._unit(x, u0, bias=u0.bias, res=skip, in_up=True)
        fused.kloop64_kernel = True
        assert calls == [("unit", (0, 64), (0, 64)), ("unit", (64, 128), (0, 64))], calls
        torch.cuda.synchronize()
        assert float((one.float() - two.float()).norm() / two.float().norm()) < 1e-2
