"""
The wave-specialised 32-channel pair (k_conv_pair32, aliby_amd/csrc/nn_conv.hip) where a workgroup walks SEVERAL tiles: the
producers request the window of tile t + 1 behind unit A's MFMAs on tile t, both sets of intermediate planes are in use, and the
last tile of a walk requests nothing.  The pair tests of test_gpu_conv.py stay at or below 256 tiles = one tile per workgroup,
where none of that runs.

Two shapes, the smallest that make a workgroup walk several tiles: (9, 224, 224) = 1152 whole tiles, 4 or 5 per workgroup; and
(70, 44, 70) = 840 tiles with ragged right and bottom edges, where the image (and with it the per-image shift) changes in
mid-walk.  Every case is bit for bit (torch.equal) against two aliby_nn_conv3x3_bf16 launches (+ aliby_nn_out_head_bf16 for the
head forms) under the ascending walk; the pair runs under the ascending and the descending walk (the prefetch follows the walk's
step).  Unit A's bias, which the producers read from LDS, and unit B's are each given and NULL; unit A takes a per-image shift
and unit B a shared one, and the other way round.
"""

import itertools

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


def _unit(engine, x, wpk, scale, shift, bias, res, pool=None):
    """One aliby_nn_conv3x3_bf16 launch, 32 -> 32 channels."""
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, H, W, _ = x.shape
    out = torch.full((n, H, W, 32), float("nan"), dtype=torch.bfloat16, device="cuda")
    _lib.check(engine.lib.aliby_nn_conv3x3_bf16(
        engine.ctx.handle, _ptr(x), _ptr(wpk), _ptr(out), _ptr(scale), _ptr(shift), 1 if shift.ndim == 2 else 0,
        _ptr(bias) if bias is not None else 0, _ptr(res) if res is not None else 0, 0, n, H, W, 32, 32,
        0, 0, 0, 0, 0, _ptr(pool) if pool is not None else 0, _stream_ptr()))
    return out


@pytest.mark.parametrize("shape", [(9, 224, 224), (70, 44, 70)])
@pytest.mark.parametrize("mode", ["plain", "pool", "head", "head_keep"])
def test_pair_walking_several_tiles_equals_two_launches(engine, order, shape, mode):
    import torch
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    n, H, W = shape
    tiles = n * ((H + 13) // 14) * ((W + 29) // 30)
    assert tiles >= 3 * 256  # every workgroup (at most 256) walks at least three tiles
    g = torch.Generator().manual_seed(n * 37 + H + len(mode))
    x = torch.randn(n, H, W, 32, generator=g).to(torch.bfloat16).cuda()
    res = torch.randn(n, H, W, 32, generator=g).to(torch.bfloat16).cuda()
    pk = []
    for _ in range(2):
        w = (torch.randn(32, 32, 3, 3, generator=g) * 0.06).float().cuda()
        p = torch.empty(32 * 32 * 9, dtype=torch.bfloat16, device="cuda")
        _lib.check(engine.lib.aliby_nn_pack_conv3x3_bf16(engine.ctx.handle, _ptr(w), 32, 32, 32, _ptr(p), _stream_ptr()))
        pk.append(p)
    sc = [(torch.rand(32, generator=g) + 0.5).float().cuda() for _ in range(2)]
    sh_image = [(torch.randn(n, 32, generator=g) * 0.2).float().cuda() for _ in range(2)]
    sh_shared = [(torch.randn(32, generator=g) * 0.2).float().cuda() for _ in range(2)]
    bi = [(torch.randn(32, generator=g) * 0.1).float().cuda() for _ in range(2)]
    hs, hb = (torch.rand(32, generator=g) + 0.5).float().cuda(), (torch.randn(32, generator=g) * 0.2).float().cuda()
    hw, hbias = (torch.randn(3, 32, generator=g) * 0.3).float().cuda(), torch.randn(3, generator=g).float().cuda()
    pool, head = mode == "pool", mode.startswith("head")

    for a_per_image, bias_a, bias_b in itertools.product((True, False), (True, False), (True, False)):
        sh = [sh_image[0], sh_shared[1]] if a_per_image else [sh_shared[0], sh_image[1]]
        ba, bb = (bi[0] if bias_a else None), (bi[1] if bias_b else None)
        case = (a_per_image, bias_a, bias_b)
        # the yardstick: two launches (+ the head kernel) under the ascending walk, computed once for both orders of the pair
        order(ASCENDING)
        mid = _unit(engine, x, pk[0], sc[0], sh[0], ba, None)
        pooled2 = torch.full((n, H // 2, W // 2, 32), float("nan"), dtype=torch.bfloat16, device="cuda") if pool else None
        want = _unit(engine, mid, pk[1], sc[1], sh[1], bb, res, pool=pooled2)
        want_head = torch.full((n, 3, H, W), float("nan"), device="cuda")
        if head:
            _lib.check(engine.lib.aliby_nn_out_head_bf16(engine.ctx.handle, _ptr(want), _ptr(hs), _ptr(hb), _ptr(hw), _ptr(hbias), n, H, W,
                                                         32, 3, _ptr(want_head), _stream_ptr()))
        for walk in (ASCENDING, DESCENDING):
            order(walk)
            out = torch.full_like(want, float("nan")) if mode != "head" else None
            pooled1 = torch.full_like(pooled2, float("nan")) if pool else None
            got_head = torch.full((n, 3, H, W), float("nan"), device="cuda")
            _lib.check(engine.lib.aliby_nn_conv3x3_pair_bf16(
                engine.ctx.handle, _ptr(x), _ptr(pk[0]), _ptr(pk[1]), _ptr(out) if out is not None else 0,
                _ptr(sc[0]), _ptr(sh[0]), 32 if sh[0].ndim == 2 else 0, _ptr(ba) if ba is not None else 0,
                _ptr(sc[1]), _ptr(sh[1]), 32 if sh[1].ndim == 2 else 0, _ptr(bb) if bb is not None else 0,
                _ptr(res), n, H, W, _ptr(pooled1) if pool else 0,
                _ptr(hs) if head else 0, _ptr(hb) if head else 0, _ptr(hw) if head else 0, _ptr(hbias) if head else 0, 3 if head else 0,
                _ptr(got_head) if head else 0, _stream_ptr()))
            torch.cuda.synchronize()
            if out is not None:
                assert torch.equal(out, want), (case, walk)
            if pool:
                assert torch.equal(pooled1, pooled2), (case, walk)
            if head:
                assert torch.equal(got_head, want_head), (case, walk)


def test_network_with_and_without_the_pairs_has_equal_bits(engine):
    """The whole network on one batch of nine 224 x 224 tiles (1152 level-0 tiles: every pair workgroup walks 4 or 5): the
    down block as a pair against its two launches, and the last block (+ output head) as a pair against its two launches."""
    import warnings

    import torch
    from aliby_amd.segment.cellpose_hip import CellposeModel

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = CellposeModel(net_dtype="bfloat16", seed=8, batch_size=9)
    net = model.fused
    assert net is not None
    tiles = torch.randn(9, 2, 224, 224, generator=torch.Generator().manual_seed(4)).cuda().contiguous()
    outs = {}
    for fused_pair, pair_head in ((True, False), (False, False), (True, True)):
        net.fused_pair, net.pair_head = fused_pair, pair_head
        y, style = net(tiles)
        torch.cuda.synchronize()
        outs[fused_pair, pair_head] = (y.clone(), style.clone())
    net.fused_pair, net.pair_head = True, False
    want_y, want_style = outs[False, False]
    assert torch.isfinite(want_y).all()
    for key in ((True, False), (True, True)):
        assert torch.equal(outs[key][0], want_y), key
        assert torch.equal(outs[key][1], want_style), key
