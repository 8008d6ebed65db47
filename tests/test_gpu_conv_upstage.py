"""
The convolutions that read their input through the nearest-neighbour 2x upsample, launch by launch through the C ABI.  The K-loop
kernels (aliby_nn_conv3x3_deep_bf16 256 -> 128, aliby_nn_conv3x3_kloop64_bf16 128 -> 64; aliby_amd/csrc/nn_conv_deep.hip) keep the
activated window in LDS at INPUT resolution and address it through aliby_amd/csrc/conv_upmap.h; aliby_nn_conv3x3_bf16 64 -> 32 is
the level-0 up block's LDS-DMA kernel.  Every entry runs at the narrowest and the widest width it is used or limited at, with
batches of 1 and 3 images (windows that span an image boundary, a last tile that is partial), a shared and a per-sample shift,
without a residual, with one at output resolution and with one read through the upsample.

  1. integer-valued data (every product and partial sum exact in fp32): bit-equal to a float64 torch computation of
     conv3x3(upsample(relu(x + shift))) + bias + res;
  2. random bf16 data: 256 -> 128 is bit-equal to the same entry point called with in_up = 0 on the materialised upsample (the same
     values enter the same MFMAs in the same order); 128 -> 64 has no such instantiation and is held against the K-split launches
     the network would otherwise run, by that path's own criterion (no further from float64 than they are).
The index map itself is checked without a GPU in tests/test_cpu_conv_upmap.py.
"""

import ctypes

import pytest

pytestmark = pytest.mark.gpu


def _limits(engine):
    from aliby_amd import _lib

    lim = (ctypes.c_int * 4)()
    _lib.check(engine.lib.aliby_nn_conv3x3_kloop_limits(lim))
    return tuple(lim)  # deep run, deep widest, kloop64 run, kloop64 widest


def _pack(engine, w):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    cout, cin = w.shape[0], w.shape[1]
    wpk = torch.empty(cout * cin * 9, dtype=torch.bfloat16, device="cuda")
    _lib.check(engine.lib.aliby_nn_pack_conv3x3_bf16(engine.ctx.handle, _ptr(w.contiguous()), cout, cin, cin, _ptr(wpk), _stream_ptr()))
    return wpk


def _launch(engine, entry, x, w, scale, shift, bias, res, res_up, in_up):
    """One launch of `entry` in ("deep", "kloop64", "conv3x3"); the output starts as NaN, so an unwritten pixel shows."""
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, ih, iw, cin = x.shape
    H, W = (2 * ih, 2 * iw) if in_up else (ih, iw)
    cout = w.shape[0]
    out = torch.full((n, H, W, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    head = (engine.ctx.handle, _ptr(x), _ptr(_pack(engine, w)), _ptr(out), _ptr(scale), _ptr(shift), 1 if shift.ndim == 2 else 0,
            _ptr(bias) if bias is not None else 0, _ptr(res) if res is not None else 0, 1 if res_up else 0, n, H, W, cin, cout, 1 if in_up else 0)
    if entry == "conv3x3":
        _lib.check(engine.lib.aliby_nn_conv3x3_bf16(*head, 0, 0, 0, 0, 0, _stream_ptr()))
    else:
        fn = engine.lib.aliby_nn_conv3x3_deep_bf16 if entry == "deep" else engine.lib.aliby_nn_conv3x3_kloop64_bf16
        _lib.check(fn(*head, _stream_ptr()))
    torch.cuda.synchronize()
    return out


def _up2(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def _ref64(x, w, scale, shift, bias, res, res_up):
    """float64 conv3x3(up2(relu(scale * x + shift) rounded to bf16)) + bias + res, NHWC, as nine shifted channel contractions."""
    import torch
    import torch.nn.functional as F

    n, ih, iw, _ = x.shape
    H, W = 2 * ih, 2 * iw
    w64 = w.bfloat16().double()
    sh = shift[:, None, None, :] if shift.ndim == 2 else shift
    a = torch.relu(x.double() * scale.double() + sh.double()).float().bfloat16().double()  # the prologue: one fp32 fma, rounded to bf16
    a = F.pad(_up2(a), (0, 0, 1, 1, 1, 1))
    y = torch.zeros((n, H, W, w.shape[0]), dtype=torch.float64, device=x.device)
    for dy in range(3):
        for dx in range(3):
            y += a[:, dy:dy + H, dx:dx + W, :] @ w64[:, :, dy, dx].t()
    if bias is not None:
        y += bias.double()
    if res is not None:
        y += (_up2(res) if res_up else res).double()
    return y


SHIFTS = ["shared", "per_sample"]
RESIDUALS = ["none", "res", "res_up"]


def _case(cin, cout, n, H, W, shift_kind, res_kind, seed, integer):
    import torch

    g = torch.Generator().manual_seed(seed)
    sshape = (n, cin) if shift_kind == "per_sample" else (cin,)
    rshape = (n, H // 2, W // 2, cout) if res_kind == "res_up" else (n, H, W, cout)
    if integer:  # small integers, scale 1, sparse +-1 weights: every partial sum is an integer far below 2^24, the result below 2^8
        x = torch.randint(-1, 3, (n, H // 2, W // 2, cin), generator=g).to(torch.bfloat16)
        w = (torch.randint(-1, 2, (cout, cin, 3, 3), generator=g) * (torch.rand(cout, cin, 3, 3, generator=g) < 12.0 / cin / 9)).float()
        scale = torch.ones(cin)
        shift = torch.randint(-1, 2, sshape, generator=g).float()
        bias = torch.randint(-2, 3, (cout,), generator=g).float()
        res = torch.randint(-3, 4, rshape, generator=g).to(torch.bfloat16)
    else:
        x = torch.randn((n, H // 2, W // 2, cin), generator=g).to(torch.bfloat16)
        w = (torch.randn((cout, cin, 3, 3), generator=g) / (3 * cin**0.5)).float()
        scale = (1 + 0.1 * torch.randn(cin, generator=g)).float()
        shift = (0.1 * torch.randn(sshape, generator=g)).float()
        bias = torch.randn(cout, generator=g).float()
        res = torch.randn(rshape, generator=g).to(torch.bfloat16)
    return x.cuda(), w.cuda(), scale.cuda(), shift.cuda(), bias.cuda(), (None if res_kind == "none" else res.cuda())


def _exact(engine, entry, cin, cout, n, H, W, shift_kind, res_kind):
    import torch

    x, w, scale, shift, bias, res = _case(cin, cout, n, H, W, shift_kind, res_kind, 7 * W + n, True)
    ref = _ref64(x, w, scale, shift, bias, res, res_kind == "res_up")
    assert float(ref.abs().max()) <= 256  # exactly representable in bf16
    out = _launch(engine, entry, x, w, scale, shift, bias, res, res_kind == "res_up", True)
    assert torch.equal(out.double(), ref), float((out.double() - ref).abs().max())


@pytest.mark.parametrize("res_kind", RESIDUALS)
@pytest.mark.parametrize("shift_kind", SHIFTS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("wide", [False, True])
def test_deep_256_to_128_is_exact_on_integer_data(engine, wide, n, shift_kind, res_kind):
    W = _limits(engine)[1] if wide else 28
    _exact(engine, "deep", 256, 128, n, W, W, shift_kind, res_kind)


@pytest.mark.parametrize("res_kind", RESIDUALS)
@pytest.mark.parametrize("shift_kind", SHIFTS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("width", ["28", "112", "widest"])
def test_kloop64_128_to_64_is_exact_on_integer_data(engine, width, n, shift_kind, res_kind):
    W = _limits(engine)[3] if width == "widest" else int(width)
    _exact(engine, "kloop64", 128, 64, n, W, W, shift_kind, res_kind)


# 64 -> 32 at the level-0 width and at a narrower one; 64 -> 64 at 112 with an even batch is the packed launch (two images side by
# side in a 224-pixel row; the library has no packed 32-channel form)
@pytest.mark.parametrize("res_kind", RESIDUALS)
@pytest.mark.parametrize("shift_kind", SHIFTS)
@pytest.mark.parametrize("cout,n,W", [(32, 1, 224), (32, 3, 224), (32, 3, 112), (64, 2, 112), (64, 4, 56)])
def test_conv3x3_64_channels_up_is_exact_on_integer_data(engine, cout, n, W, shift_kind, res_kind):
    _exact(engine, "conv3x3", 64, cout, n, W, W, shift_kind, res_kind)


@pytest.mark.parametrize("res_kind", RESIDUALS)
@pytest.mark.parametrize("shift_kind", SHIFTS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("W", [28, 56])
def test_deep_256_to_128_has_the_bits_of_the_launch_on_the_materialised_upsample(engine, W, n, shift_kind, res_kind):
    import torch

    x, w, scale, shift, bias, res = _case(256, 128, n, W, W, shift_kind, res_kind, 11 * W + n, False)
    through = _launch(engine, "deep", x, w, scale, shift, bias, res, res_kind == "res_up", True)
    plain = _launch(engine, "deep", _up2(x).contiguous(), w, scale, shift, bias, res, res_kind == "res_up", False)
    assert not torch.isnan(through.float()).any()
    assert torch.equal(through.view(torch.int16), plain.view(torch.int16))


def _k_split(engine, x, w, scale, shift, bias, res, res_up):
    """The two launches the K-loop launch replaces (FusedUNet._unit's K split): input channels 0-63, then 64-127 adding to the first
    launch's bf16 output; the bias rides in the last one."""
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, ih, iw, cin = x.shape
    H, W, cout = 2 * ih, 2 * iw, w.shape[0]
    out = torch.full((n, H, W, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    cur, cur_up = res, res_up
    for k0 in range(0, cin, 64):
        last = k0 + 64 == cin
        sh = shift[..., k0:k0 + 64].contiguous()
        _lib.check(engine.lib.aliby_nn_conv3x3_bf16(
            engine.ctx.handle, _ptr(x), _ptr(_pack(engine, w[:, k0:k0 + 64].contiguous())), _ptr(out), _ptr(scale[k0:k0 + 64].contiguous()), _ptr(sh),
            1 if sh.ndim == 2 else 0, _ptr(bias) if last else 0, _ptr(cur) if cur is not None else 0, 1 if cur_up else 0, n, H, W, 64, cout, 1, cin,
            k0, 0, 0, 0, _stream_ptr()))
        cur, cur_up = out, False
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("res_kind", RESIDUALS)
@pytest.mark.parametrize("shift_kind", SHIFTS)
@pytest.mark.parametrize("n,W", [(1, 28), (3, 28), (1, 112), (3, 112)])
def test_kloop64_random_data_is_no_further_from_fp64_than_the_k_split_launches(engine, n, W, shift_kind, res_kind):
    """One bf16 rounding (of the result) against two (the partial sum after 64 channels, then the result)."""
    x, w, scale, shift, bias, res = _case(128, 64, n, W, W, shift_kind, res_kind, 13 * W + n, False)
    ref = _ref64(x, w, scale, shift, bias, res, res_kind == "res_up")
    one = _launch(engine, "kloop64", x, w, scale, shift, bias, res, res_kind == "res_up", True).double()
    two = _k_split(engine, x, w, scale, shift, bias, res, res_kind == "res_up").double()
    err_one, err_two = float((one - ref).norm() / ref.norm()), float((two - ref).norm() / ref.norm())
    print(f"rel-L2 vs float64: K-loop {err_one:.3e}, K-split launches {err_two:.3e}")
    assert err_one <= err_two, (err_one, err_two)
