"""
Tile order of the persistent convolution launches (aliby_nn_conv_order; tile_walk in aliby_amd/csrc/conv_launch.h): every XCD
walks its eighth of a launch's tiles upwards, downwards, or in the direction opposite to the context's previous launch.  The
order changes WHEN a tile is computed, never what it computes, so the yardstick is the ascending walk, which the other conv
suites tie to their references: descending, and two launches in a row in alternate mode (one of each direction), must
reproduce its outputs bit for bit, for every entry point and form the network launches.

Three sizes per form, the smallest at which a walk can go wrong: fewer than 8 tiles (some XCDs' ranges are empty); a tile
count that is no multiple of 8 (the last XCD's range is short, or empty); and more than 16 x the form's workgroups per XCD
(1024 tiles where two workgroups share a CU, 512 where one does), so that at least one workgroup walks three tiles and the
next-tile prefetch and the end of the walk are exercised in both directions.  Random data, a per-sample shift and a residual
wherever the form takes them.
"""

import pytest

pytestmark = pytest.mark.gpu

ALTERNATE, ASCENDING, DESCENDING = 0, 1, 2


def _set_order(engine, mode):
    from aliby_amd import _lib

    _lib.check(engine.lib.aliby_nn_conv_order(engine.ctx.handle, mode))


@pytest.fixture
def order(engine):
    """Sets the context's mode; a new context's mode (alternate) is back in place after the test."""
    yield lambda mode: _set_order(engine, mode)
    _set_order(engine, ALTERNATE)


def _gen(seed):
    import torch

    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape, std=1.0, dtype=None):
    import torch

    t = torch.randn(shape, device="cuda", generator=g) * std
    return t.to(dtype).contiguous() if dtype is not None else t.contiguous()


def _pack(engine, w, taps=9, cin_pad=None):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    cout, cin = w.shape[0], w.shape[1]
    cin_pad = cin_pad or cin
    pk = torch.empty(cout * cin_pad * taps, dtype=torch.bfloat16, device="cuda")
    fn = engine.lib.aliby_nn_pack_conv3x3_bf16 if taps == 9 else engine.lib.aliby_nn_pack_conv1x1_bf16
    _lib.check(fn(engine.ctx.handle, _ptr(w.contiguous()), cout, cin, cin_pad, _ptr(pk), _stream_ptr()))
    return pk


def _unit_operands(engine, g, n, H, W, cin, cout, in_up):
    """x, packed 3x3 weights, scale, per-sample shift, bias and a full-resolution residual of one convolution unit."""
    import torch

    ih, iw = (H // 2, W // 2) if in_up else (H, W)
    x = _randn(g, n, ih, iw, cin, dtype=torch.bfloat16)
    wpk = _pack(engine, _randn(g, cout, cin, 3, 3, std=1.0 / (3 * cin**0.5)))
    scale = 1 + 0.1 * _randn(g, cin)
    shift = _randn(g, n, cin, std=0.2)
    bias = _randn(g, cout, std=0.1)
    res = _randn(g, n, H, W, cout, dtype=torch.bfloat16)
    return x, wpk, scale, shift, bias, res


def _head_operands(g, O=3):
    import torch

    return (torch.rand(32, device="cuda", generator=g) + 0.5).contiguous(), _randn(g, 32, std=0.2), _randn(g, O, 32, std=0.3), _randn(g, O)


def _nan(*shape, dtype=None):
    import torch

    return torch.full(shape, float("nan"), dtype=dtype or torch.bfloat16, device="cuda")


# ---- the forms: each returns a function that makes ONE launch into fresh NaN-filled outputs and returns them
def _form_unit(engine, g, shape, cin, cout, in_up=False, res=True, pool=False):
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, H, W = shape
    x, wpk, scale, shift, bias, r = _unit_operands(engine, g, n, H, W, cin, cout, in_up)

    def launch():
        out = _nan(n, H, W, cout)
        pooled = _nan(n, H // 2, W // 2, cout) if pool else None
        _lib.check(engine.lib.aliby_nn_conv3x3_bf16(
            engine.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(scale), _ptr(shift), 1, _ptr(bias), _ptr(r) if res else 0, 0, n, H, W,
            cin, cout, 1 if in_up else 0, 0, 0, 0, 0, _ptr(pooled) if pool else 0, _stream_ptr()))
        return [out] + ([pooled] if pool else [])

    return launch


def _form_proj(engine, g, shape, cin, pc):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, H, W = shape
    x, wpk, scale, shift, bias, _ = _unit_operands(engine, g, n, H, W, cin, cin, False)
    xin = _randn(g, n, H, W, pc, dtype=torch.bfloat16)
    ppk = _pack(engine, _randn(g, cin, pc, std=0.3), taps=1, cin_pad=16 if cin == 32 else 32)

    def launch():
        out = _nan(n, H, W, cin)
        _lib.check(engine.lib.aliby_nn_conv3x3_proj_bf16(engine.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(scale), _ptr(shift), 1, _ptr(bias),
                                                         n, H, W, cin, cin, _ptr(xin), _ptr(ppk), pc, _stream_ptr()))
        return [out]

    return launch


def _form_head(engine, g, shape):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, H, W = shape
    x, wpk, scale, shift, bias, r = _unit_operands(engine, g, n, H, W, 32, 32, False)
    hs, hb, hw, hbias = _head_operands(g)

    def launch():
        out, y = _nan(n, H, W, 32), _nan(n, 3, H, W, dtype=torch.float32)
        _lib.check(engine.lib.aliby_nn_conv3x3_head_bf16(
            engine.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(scale), _ptr(shift), 1, _ptr(bias), _ptr(r), 0, n, H, W, 32, 32, _ptr(hs),
            _ptr(hb), _ptr(hw), _ptr(hbias), 3, _ptr(y), _stream_ptr()))
        return [out, y]

    return launch


def _form_pair(engine, g, shape, mode):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, H, W = shape
    x, wa, sa, ha, ba, r = _unit_operands(engine, g, n, H, W, 32, 32, False)
    _, wb, sb, _, bb, _ = _unit_operands(engine, g, 1, 2, 2, 32, 32, False)
    hb_shared = _randn(g, 32, std=0.2)  # unit B's shift: shared, as in the network
    hs, hb, hw, hbias = _head_operands(g)
    pool, head = mode == "pool", mode == "head"

    def launch():
        out = _nan(n, H, W, 32)
        pooled = _nan(n, H // 2, W // 2, 32) if pool else None
        y = _nan(n, 3, H, W, dtype=torch.float32) if head else None
        _lib.check(engine.lib.aliby_nn_conv3x3_pair_bf16(
            engine.ctx.handle, _ptr(x), _ptr(wa), _ptr(wb), _ptr(out), _ptr(sa), _ptr(ha), 1, _ptr(ba), _ptr(sb), _ptr(hb_shared), 0, _ptr(bb),
            _ptr(r), n, H, W, _ptr(pooled) if pool else 0, _ptr(hs) if head else 0, _ptr(hb) if head else 0, _ptr(hw) if head else 0,
            _ptr(hbias) if head else 0, 3 if head else 0, _ptr(y) if head else 0, _stream_ptr()))
        return [t for t in (out, pooled, y) if t is not None]

    return launch


def _form_first_pair(engine, g, shape):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, H, W = shape
    cin = 2
    tiles = _randn(g, n, cin, H, W, std=2.0)
    s0, h0 = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    s0[:cin] = torch.rand(cin, device="cuda", generator=g) + 0.5
    h0[:cin] = _randn(g, cin, std=0.3)
    w0 = _randn(g, 32, cin, 3, 3, std=0.3).to(torch.bfloat16).float().contiguous()  # bf16-representable, as the entry point expects
    _, wpk1, s1, _, b1, _ = _unit_operands(engine, g, 1, 2, 2, 32, 32, False)
    h1 = _randn(g, 32, std=0.2)
    wp = torch.zeros(32, 8, device="cuda")
    wp[:, :cin] = _randn(g, 32, cin, std=0.4)
    ppk = _pack(engine, wp, taps=1, cin_pad=16)

    def launch():
        out = _nan(n, H, W, 32)
        _lib.check(engine.lib.aliby_nn_first_pair_bf16(engine.ctx.handle, _ptr(tiles), n, cin, H, W, _ptr(s0), _ptr(h0), _ptr(w0), _ptr(wpk1), _ptr(s1),
                                                       _ptr(h1), _ptr(b1), _ptr(ppk), _ptr(out), _stream_ptr()))
        return [out]

    return launch


def _form_deep(engine, g, shape, cin, cout, in_up=False, entry="aliby_nn_conv3x3_deep_bf16"):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, H, W = shape
    x, wpk, scale, shift, bias, r = _unit_operands(engine, g, n, H, W, cin, cout, in_up)
    if entry == "aliby_nn_conv3x3_deep16_bf16":  # its own fragment order
        w = _randn(g, cout, cin, 3, 3, std=1.0 / (3 * cin**0.5))
        wpk = torch.empty(cout * cin * 9, dtype=torch.bfloat16, device="cuda")
        _lib.check(engine.lib.aliby_nn_pack_conv3x3_deep16_bf16(engine.ctx.handle, _ptr(w), cout, cin, _ptr(wpk), _stream_ptr()))

    def launch():
        out = _nan(n, H, W, cout)
        _lib.check(getattr(engine.lib, entry)(engine.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(scale), _ptr(shift), 1, _ptr(bias), _ptr(r), 0,
                                              n, H, W, cin, cout, 1 if in_up else 0, _stream_ptr()))
        return [out]

    return launch


# tile shapes (aliby_amd/csrc/nn_conv.hip, nn_conv_deep.hip) behind the sizes: the register-staged unit's tiles are 32 pixels
# wide and 8, 16 or 32 rows tall, two workgroups per CU (64 per XCD); packed launches take 224 / W images per tile row; the
# pair kernels' tiles are 14 x 30, one workgroup per CU (32 per XCD); a deep tile is 224 positions (448 in kloop64) of the tall
# image x 128 output channels, two workgroups per CU.  The tile counts are in the comments
SMALL, ODD = (1, 20, 40), (3, 44, 70)  # 2..6 and 27..54 tiles of the 32-pixel-wide units; 1 and 36 of the pair kernels
FORMS = {
    "plain32": (lambda e, g, s: _form_unit(e, g, s, 32, 32), [SMALL, ODD, (21, 224, 224)]),  # 1029
    "plain64": (lambda e, g, s: _form_unit(e, g, s, 64, 64), [SMALL, ODD, (29, 96, 96)]),  # 1044
    "packed64_56": (lambda e, g, s: _form_unit(e, g, s, 64, 64), [(4, 8, 56), (4, 56, 56), (84, 56, 56)]),  # 7, 49, 1029
    "packed64_112": (lambda e, g, s: _form_unit(e, g, s, 64, 64), [(2, 16, 112), (2, 112, 112), (42, 112, 112)]),  # 7, 49, 1029
    "pool32_64": (lambda e, g, s: _form_unit(e, g, s, 32, 64, res=False, pool=True), [(2, 8, 112), (2, 112, 112), (22, 112, 112)]),  # 7, 98, 1078
    "proj64": (lambda e, g, s: _form_proj(e, g, s, 64, 32), [SMALL, ODD, (19, 112, 112)]),  # 1064
    "proj32": (lambda e, g, s: _form_proj(e, g, s, 32, 8), [SMALL, ODD, (11, 224, 224)]),  # 1078
    "head": (_form_head, [SMALL, ODD, (21, 224, 224)]),  # 1029
    "up_dma64_32": (lambda e, g, s: _form_unit(e, g, s, 64, 32, in_up=True), [SMALL, ODD, (6, 224, 224)]),  # 1176
    "pair": (lambda e, g, s: _form_pair(e, g, s, "plain"), [(1, 10, 6), ODD, (5, 224, 224)]),  # 640: 80 per XCD, slots walk 3 or 2
    "pair_pool": (lambda e, g, s: _form_pair(e, g, s, "pool"), [(1, 10, 6), ODD, (5, 224, 224)]),
    "pair_head": (lambda e, g, s: _form_pair(e, g, s, "head"), [(1, 10, 6), ODD, (5, 224, 224)]),
    "first_pair": (_form_first_pair, [(1, 10, 6), ODD, (5, 224, 224)]),
    "deep64_128": (lambda e, g, s: _form_deep(e, g, s, 64, 128), [(1, 14, 28), (5, 56, 56), (70, 56, 56)]),  # 2, 74, 1033
    "deep128_128": (lambda e, g, s: _form_deep(e, g, s, 128, 128), [(1, 14, 28), (5, 56, 56), (70, 56, 56)]),
    "deep256_256": (lambda e, g, s: _form_deep(e, g, s, 256, 256), [(1, 14, 28), (9, 28, 28), (132, 28, 28)]),  # two halves per run: 4, 70, 1026
    "deep256_128_up": (lambda e, g, s: _form_deep(e, g, s, 256, 128, in_up=True), [(1, 14, 28), (5, 56, 56), (70, 56, 56)]),
    "deep16_256_256": (lambda e, g, s: _form_deep(e, g, s, 256, 256, entry="aliby_nn_conv3x3_deep16_bf16"),
                       [(1, 14, 28), (9, 28, 28), (132, 28, 28)]),
    "kloop64": (lambda e, g, s: _form_deep(e, g, s, 128, 64, in_up=True, entry="aliby_nn_conv3x3_kloop64_bf16"),
                [(1, 32, 32), (2, 112, 112), (36, 112, 112)]),  # 3, 58, 1035
}
CASES = [(name, shape) for name, (_, shapes) in FORMS.items() for shape in shapes]


def _bits(t):
    import torch

    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check_orders(engine, order, launch, what):
    import torch

    order(ASCENDING)
    want = launch()
    for t in want:
        assert not bool(torch.isnan(t).any()), f"{what}: the ascending walk left output unwritten"
    order(DESCENDING)
    runs = {"descending": launch()}
    order(ALTERNATE)  # the alternation restarts: one launch upwards, then one downwards
    runs["alternate, first launch"] = launch()
    runs["alternate, second launch"] = launch()
    torch.cuda.synchronize()
    for mode, got in runs.items():
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(_bits(a), _bits(b)), f"{what}, {mode}: output {k} differs from the ascending walk"


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s in CASES])
def test_every_tile_order_gives_the_bits_of_the_ascending_walk(engine, order, name, shape):
    make = FORMS[name][0]
    launch = make(engine, _gen(sum(map(ord, name)) + shape[0]), shape)
    _check_orders(engine, order, launch, f"{name} {shape}")


@pytest.mark.parametrize("shape", [(1, 14, 28), (9, 28, 28), (70, 28, 28)])  # 4, 70 and 546 tiles; one workgroup per CU: 3 per slot
def test_loader_specialised_deep_form_in_every_tile_order(engine, order, monkeypatch, shape):
    """k_conv3x3_deep_ls (ALIBY_DEEP_LS=1, read per call): its loader waves name the tile after next."""
    monkeypatch.setenv("ALIBY_DEEP_LS", "1")
    _check_orders(engine, order, _form_deep(engine, _gen(77 + shape[0]), shape, 256, 256), f"deep_ls {shape}")


def test_unknown_mode_is_refused_and_changes_nothing(engine, order):
    from aliby_amd import _lib

    for mode in (-1, 3):
        with pytest.raises(ValueError, match="conv_order"):
            _lib.check(engine.lib.aliby_nn_conv_order(engine.ctx.handle, mode))


def test_whole_network_forward_has_the_same_bits_in_every_mode(engine, order):
    import torch
    from aliby_amd.segment.fused_unet import FusedUNet
    from aliby_amd.segment.unet import build_network

    fused = FusedUNet(build_network(seed=5, device="cuda"), engine)
    tiles = _randn(_gen(3), 3, 2, 224, 224)
    outs = {}
    for name, mode in (("ascending", ASCENDING), ("descending", DESCENDING), ("alternate", ALTERNATE)):
        order(mode)
        y, style = fused(tiles)
        torch.cuda.synchronize()
        outs[name] = (y.clone(), style.clone())
    assert bool(torch.isfinite(outs["ascending"][0]).all())
    for name in ("descending", "alternate"):
        assert torch.equal(_bits(outs[name][0]), _bits(outs["ascending"][0])), f"y, {name}"
        assert torch.equal(_bits(outs[name][1]), _bits(outs["ascending"][1])), f"style, {name}"
