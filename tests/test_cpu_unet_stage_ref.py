"""The float64 stage references of tests/unet_stage_ref.py checked against the module itself (no GPU): composed with the rounding
switched off they ARE ResidualUNet.forward, and the per-element checker accepts their own bf16 outputs and rejects the local
errors a global norm hides."""

import pytest
import torch

from tests import unet_stage_ref as sr


def _net(seed):
    from aliby_amd.segment.unet import build_network

    net = build_network(seed=seed, device="cpu")
    g = torch.Generator(device="cpu").manual_seed(seed + 100)
    with torch.no_grad():
        for m in net.modules():  # non-trivial BatchNorm, so that every folded term matters
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    return net


def _tiles(n, h, w, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, 2, h, w, generator=g, dtype=torch.float64)
    return x * torch.linspace(0.5, 2.0, n, dtype=torch.float64)[:, None, None, None] + torch.arange(n, dtype=torch.float64)[:, None, None, None] * 0.3


@pytest.mark.parametrize("h,w", [(32, 32), (24, 40)])
def test_stage_references_compose_to_the_module_forward(h, w):
    net = _net(3)
    x = _tiles(2, h, w, 7)
    y_mod, s_mod = sr.module_forward(net, x, round_weights=False)
    y, s, _ = sr.forward(net, x, rnd=False)
    assert float((y - y_mod).norm() / y_mod.norm()) < 1e-12
    assert float((s - s_mod).norm() / s_mod.norm()) < 1e-12


def _stages(net, x):
    """A few stages of every form with rounding on, from the rounded forward's own intermediates: (name, ref, S, m)."""
    _, sv, st = sr.forward(net, x, rnd=True)
    d0, d1, d2, u0, u1 = net.down[0], net.down[1], net.down[2], net.up[0], net.up[1]
    sh = sr.shifts_of(net, sr.style_shifts(net, sv)[0])
    b = lambda seq: sr.conv_w(seq, False)[1]  # noqa: E731
    p1 = torch.nn.functional.max_pool2d(st["d0.x2"], 2, 2)
    p2 = torch.nn.functional.max_pool2d(st["d1.x2"], 2, 2)
    out = []
    out.append(("first_pair", *sr.first_pair(x, d0), 1))
    out.append(("pair", *sr.pair(st["d0.x1"], d0.conv[2], d0.conv[3], b(d0.conv[2]), b(d0.conv[3]), st["d0.x1"]), 1))
    out.append(("unit", *sr.unit(p1, d1.conv[0], b(d1.conv[0])), 0))
    out.append(("unit_proj", *sr.unit_proj(st["d1.c0"], d1.conv[1], b(d1.conv[1]), p1, d1.proj), 0))
    out.append(("proj", *sr.proj(p2, d2.proj), 0))
    out.append(("unit_ksplit", *sr.unit(st["d2.x1"], d2.conv[2], b(d2.conv[2]), k_slices=2), 1))
    out.append(("unit_styled_up", *sr.unit(st["u1.c0s"], u1.conv1.conv, b(u1.conv1.conv) + sr.proj_params(u1.proj, True)[1],
                                          shift=sh[(1, 1)], res=sr.proj(st["u2.x"], u1.proj)[0], res_up=True), 0))
    out.append(("unit_head", *sr.unit_head(st["u0.c2"], u0.conv3.conv, b(u0.conv3.conv), st["u0.x1"], net.output, shift=sh[(0, 3)]), 1))
    return out, sh, st


def test_checker_accepts_the_references_own_outputs():
    net = _net(4)
    x = _tiles(2, 32, 32, 8)
    stages, _, _ = _stages(net, x)
    for name, ref, S, m in stages:
        worst, equal = sr.check(name, ref.clone(), ref, S, m)
        assert worst == 0.0 and equal == 1.0, name


def test_bf16_rounding_is_round_to_nearest_even():
    one = torch.tensor([1.0], dtype=torch.float64)
    ulp = 2.0 ** -7
    vals = torch.tensor([1 + ulp / 2, 1 + 1.5 * ulp, 1 + ulp / 2 + 2 ** -30, -(1 + ulp / 2), 0.0, 3.0e-3], dtype=torch.float64)
    want = torch.tensor([1.0, 1 + 2 * ulp, 1 + ulp, -1.0, 0.0, float(torch.tensor(3.0e-3).to(torch.bfloat16).double())], dtype=torch.float64)
    assert torch.equal(sr.bf16(vals), want)
    assert float(sr.ulp_bf16(one)) == ulp and float(sr.ulp_bf16(torch.tensor([0.0], dtype=torch.float64))) == 0.0
    g = torch.Generator().manual_seed(0)
    r = torch.randn(10000, generator=g, dtype=torch.float32).double()  # exactly representable in fp32: one rounding either way
    assert torch.equal(sr.bf16(r), r.float().to(torch.bfloat16).double())


def _rejects(name, out, ref, S, m):
    with pytest.raises(AssertionError, match="outside the bound"):
        sr.check(name, out, ref, S, m)


def test_checker_rejects_local_errors():
    net = _net(5)
    x = _tiles(2, 32, 32, 9)
    _, sv, st = sr.forward(net, x, rnd=True)
    d1 = net.down[1]
    p1 = torch.nn.functional.max_pool2d(st["d0.x2"], 2, 2)
    bias = sr.conv_w(d1.conv[0], False)[1]
    ref, S = sr.unit(p1, d1.conv[0], bias)
    # one border row replaced by its neighbour
    bad = ref.clone()
    bad[1, :, 0, :] = bad[1, :, 1, :]
    _rejects("border row", bad, ref, S, 0)
    # one border column replaced by its neighbour
    bad = ref.clone()
    bad[0, :, :, -1] = bad[0, :, :, -2]
    _rejects("border column", bad, ref, S, 0)
    # one channel's bias dropped
    c = int(bias.abs().argmax())
    nob = bias.clone()
    nob[c] = 0.0
    bad, _ = sr.unit(p1, d1.conv[0], nob)
    _rejects("bias dropped", bad, ref, S, 0)
    # the style shifts of two samples swapped, in a styled unit of the up path
    u1 = net.up[1]
    sh = sr.shifts_of(net, sr.style_shifts(net, sv)[0])[(1, 2)]
    b2 = sr.conv_w(u1.conv2.conv, False)[1]
    ref, S = sr.unit(st["u1.x1"], u1.conv2.conv, b2, shift=sh)
    bad, _ = sr.unit(st["u1.x1"], u1.conv2.conv, b2, shift=sh.flip(0))
    _rejects("style shifts swapped", bad, ref, S, 0)
