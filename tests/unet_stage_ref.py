"""
Float64 references of the fused U-Net's launches, one per launch form of `FusedUNet.__call__` (aliby_amd/segment/fused_unet.py),
and the per-element checker that compares a kernel's output with them.

Every parameter is read from the `nn.Module` (aliby_amd/segment/unet.py): conv weights and biases, BatchNorm statistics, the
styled units' `full` Linear.  Nothing is taken from FusedUNet's folded tensors (`shift1_b0`, `pb1`, `_Proj`, `style_w` /
`style_b`), so the folding is under test too.  The functions work on float64 NCHW tensors; `rnd=True` rounds to bf16 (round to
nearest even, straight from float64) at exactly the points where the kernels round, and nowhere else:

  * conv weights (k_pack_conv3x3 / k_pack_conv1x1: cv_f2bf of the fp32 OIHW weights; first layer: FusedUNet.first_w);
  * projection weights after the BatchNorm is folded into them (`_Proj`: w * s, then the pack kernel's cv_f2bf);
  * the prologue activation bf16(relu(scale * x + shift)) (nn_conv.hip conv_act8, nn_conv_deep.hip dc_act8; first layer:
    k_conv_first_pair "separate multiply and add, ReLU in float, then round to bf16");
  * every tensor a kernel stores (nn_conv.hip conv_store / the pooled epilogue's cv_pack2, nn_conv1x1.hip p1_pack2);
  * the intermediate the pair keeps in LDS (k_conv_pair32: "bf16 as the two-launch path stores it, then B's prologue");
  * the partial sums between K-split launches (FusedUNet._unit: each K-slice adds to the previous one through OUT, in place);
  * `c0` of the first layer, without its bias (k_conv_first_pair: cv_pack2 of the accumulator, the bias rides in `shift1_b0`);
  * the raw tiles the first pair's projection reads (k_conv_first_pair: rawPh = cv_pack2(v));
  * the standalone projection's output, without its bias (k_conv1x1 is called with bias = 0; the consumer adds `pb1`);
  * the last unit's output before the output head (head_from_acc: cv_pack2 of the accumulators, then the head's prologue).

Each stage function returns (ref, S): S is the same stage evaluated on absolute values — |activation| * |weights| + |bias| +
|residual|, propagated through every internal rounding point — the scale of the accumulation error in the bound of `check`.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------- rounding
def bf16(x: torch.Tensor) -> torch.Tensor:
    """Round float64 to the nearest bf16 value, ties to even, in one step (no detour through float32: double rounding)."""
    m, e = torch.frexp(x)  # x = m * 2^e, 0.5 <= |m| < 1: 8 significant bits are kept
    return torch.ldexp(torch.round(torch.ldexp(m, torch.full_like(e, 8))), e - 8)  # torch.round: half to even


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 values at |x| (0 at x = 0)."""
    _, e = torch.frexp(x)
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 8))


def _r(x, rnd):
    return bf16(x) if rnd else x


# ---------------------------------------------------------------------------------------------------------- parameters
def bn_affine(bn):
    """Eval-mode BatchNorm as scale, shift (float64)."""
    s = bn.weight.detach().to(F64) / torch.sqrt(bn.running_var.detach().to(F64) + bn.eps)
    t = bn.bias.detach().to(F64) - bn.running_mean.detach().to(F64) * s
    return s, t


def conv_w(seq, rnd):
    """(weight, bias) of the Conv2d that ends a BN -> [ReLU] -> Conv unit."""
    conv = seq[-1]
    return _r(conv.weight.detach().to(F64), rnd), conv.bias.detach().to(F64)


def proj_params(seq, rnd):
    """BN -> 1x1 conv folded: (weight [O, I, 1, 1], bias).  The weights are rounded after folding (as `_Proj` packs them)."""
    s, t = bn_affine(seq[0])
    w = seq[-1].weight.detach().to(F64)
    b = seq[-1].bias.detach().to(F64) + w[:, :, 0, 0] @ t
    return _r(w * s[None, :, None, None], rnd), b


def _c(v):
    return v[None, :, None, None]


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def _act(x, seq, shift, rnd):
    """bf16(relu(scale * x + shift)); `shift` [N, C] per sample (styled units) or None (the BatchNorm's own)."""
    s, t = bn_affine(seq[0])
    sh = _c(t) if shift is None else shift[:, :, None, None]
    return _r(torch.relu(_c(s) * x + sh), rnd)


def _act_abs(xa, seq, shift):
    """Majorant of |scale * x + shift| for |x| <= xa."""
    s, t = bn_affine(seq[0])
    sh = _c(t).abs() if shift is None else shift.abs()[:, :, None, None]
    return _c(s).abs() * xa + sh


def _conv(a, w):
    return F.conv2d(a, w, padding=w.shape[-1] // 2)


def _sconv(a, w):
    """A term of S (|a| * |w|, both non-negative): in float32, whose 1e-7 relative error is nothing to a bound that S scales."""
    return _conv(a.float(), w.float()).to(F64)


# ---------------------------------------------------------------------------------------------------------- stages
def first_pair(tiles, blk, rnd=True):
    """k_conv_first_pair: x1 = conv1(act1(c0 + b0)) + b1 + proj(tiles); c0 = conv0(act0(tiles)) without its bias.
    `blk` is the first DownBlock; tiles float [N, cin, H, W]."""
    s0, t0 = bn_affine(blk.conv[0][0])
    w0, b0 = conv_w(blk.conv[0], rnd)
    w1, b1 = conv_w(blk.conv[1], rnd)
    wp, bp = proj_params(blk.proj, rnd)
    x = tiles.to(F64)
    a0 = _r(torch.relu(_c(s0) * x + _c(t0)), rnd)
    c0 = _r(_conv(a0, w0), rnd)
    c0_abs = _sconv(a0.abs(), w0.abs())
    a1 = _act(c0 + _c(b0), blk.conv[1], None, rnd)
    xr = _r(x, rnd)
    ref = _r(_conv(a1, w1) + _c(b1) + _conv(xr, wp) + _c(bp), rnd)
    S = _sconv(_act_abs(c0_abs + _c(b0).abs(), blk.conv[1], None), w1.abs()) + _c(b1).abs() + _sconv(xr.abs(), wp.abs()) + _c(bp).abs()
    return ref, S


def unit(x, seq, bias, shift=None, res=None, res_up=False, in_up=False, k_slices=1, rnd=True):
    """k_conv3x3 / k_conv3x3_deep / the K-split launches: conv3x3(act(up?(x))) + bias + up?(res), pooled outside.
    k_slices > 1: the reduction runs as k_slices launches of cin / k_slices channels, each rounding its partial sum to bf16
    into OUT, which the next launch reads as its residual; the bias comes with the last launch (FusedUNet._unit)."""
    w, _ = conv_w(seq, rnd)
    xi = _up(x) if in_up else x
    a = _act(xi, seq, shift, rnd)
    r = None if res is None else (_up(res) if res_up else res)
    cin = a.shape[1]
    ks = cin // k_slices
    acc = torch.zeros((), dtype=F64) if r is None else r
    for j in range(k_slices):
        part = _conv(a[:, j * ks:(j + 1) * ks], w[:, j * ks:(j + 1) * ks])
        acc = acc + part + (_c(bias) if j == k_slices - 1 else 0.0)
        if k_slices > 1:
            acc = _r(acc, rnd)
    ref = _r(acc, rnd)
    S = _sconv(a.abs(), w.abs()) + _c(bias).abs() + (0.0 if r is None else r.abs())
    return ref, S


def unit_proj(x, seq, bias, x_in, proj_seq, rnd=True):
    """k_conv3x3 with the block's 1x1 projection as extra k-steps: conv3x3(act(x)) + bias + proj(x_in).
    `bias` is the unit's own; the projection's folded bias is added here."""
    wp, bp = proj_params(proj_seq, rnd)
    w, _ = conv_w(seq, rnd)
    a = _act(x, seq, None, rnd)
    ref = _r(_conv(a, w) + _conv(x_in, wp) + _c(bias + bp), rnd)
    S = _sconv(a.abs(), w.abs()) + _sconv(x_in.abs(), wp.abs()) + _c(bias + bp).abs()
    return ref, S


def pair(x, seq_a, seq_b, bias_a, bias_b, res, shift_a=None, shift_b=None, rnd=True):
    """k_conv_pair32: conv_b(act_b(bf16(conv_a(act_a(x)) + bias_a))) + bias_b + res, the intermediate kept in LDS."""
    wa, _ = conv_w(seq_a, rnd)
    wb, _ = conv_w(seq_b, rnd)
    aa = _act(x, seq_a, shift_a, rnd)
    mid = _r(_conv(aa, wa) + _c(bias_a), rnd)
    ab = _act(mid, seq_b, shift_b, rnd)
    ref = _r(_conv(ab, wb) + _c(bias_b) + res, rnd)
    mid_abs = _sconv(aa.abs(), wa.abs()) + _c(bias_a).abs()
    S = _sconv(_act_abs(mid_abs, seq_b, shift_b), wb.abs()) + _c(bias_b).abs() + res.abs()
    return ref, S


def unit_head(x, seq, bias, res, out_seq, shift=None, rnd=True):
    """k_conv3x3 with the output head in its epilogue: y = conv1x1(act_o(bf16(conv3x3(act(x)) + bias + res))) + b_o,
    float32 output (not rounded)."""
    u, Su = unit(x, seq, bias, shift=shift, res=res, rnd=rnd)
    wo, bo = conv_w(out_seq, rnd)
    ao = _act(u, out_seq, None, rnd)
    y = _conv(ao, wo) + _c(bo)
    S = _sconv(_act_abs(Su, out_seq, None), wo.abs()) + _c(bo).abs()
    return y, S


def proj(x, proj_seq, rnd=True):
    """k_conv1x1 (standalone projection): bf16(conv1x1(x, w * s)) WITHOUT the folded bias, which its consumer adds."""
    wp, _ = proj_params(proj_seq, rnd)
    return _r(_conv(x, wp), rnd), _sconv(x.abs(), wp.abs())


def style(deep):
    """k_style: the L2-normalised spatial mean of the deepest map.  Returns (style [N, C], scale of the terms [N, C]): the scale
    is sum |x| / (P * norm), the size of the terms the fp32 mean adds up (reported beside the per-element relative error)."""
    d = deep.to(F64)
    m = d.mean(dim=(2, 3))
    nrm = torch.sqrt((m * m).sum(dim=1, keepdim=True))
    return m / nrm, d.abs().mean(dim=(2, 3)) / nrm


def style_shifts(net, style_vec):
    """The per-sample shift of every styled unit: scale * (full(style) + full.bias) + shift of the unit's BatchNorm, in the
    order of `net.up` (conv1, conv2, conv3 of each block).  Returns (shifts [N, sum C], scale of the terms [N, sum C])."""
    st = style_vec.to(F64)
    out, mag = [], []
    for blk in net.up:
        for su in (blk.conv1, blk.conv2, blk.conv3):
            s, t = bn_affine(su.conv[0])
            W = su.full.weight.detach().to(F64)
            b = su.full.bias.detach().to(F64)
            out.append(s * (st @ W.t() + b) + t)
            mag.append(s.abs() * (st.abs() @ W.abs().t() + b.abs()) + t.abs())
    return torch.cat(out, dim=1), torch.cat(mag, dim=1)


def shifts_of(net, shifts):
    """Split `style_shifts` output into {(up block index, styled unit 1..3): [N, C]}."""
    out, off = {}, 0
    for i, blk in enumerate(net.up):
        for k, su in ((1, blk.conv1), (2, blk.conv2), (3, blk.conv3)):
            c = su.full.out_features
            out[(i, k)] = shifts[:, off:off + c]
            off += c
    return out


# ---------------------------------------------------------------------------------------------------------- the whole forward
def forward(net, x, rnd=True):
    """The fused forward's launch sequence composed from the stage references (default FusedUNet: fused first pair,
    level-0 pairs, unit + head; every stage single-launch, i.e. no K-split rounding).  Returns (y, style, stages):
    stages maps a stage name to its float64 output, for the checker's own tests."""
    st = {}
    d0 = net.down[0]
    x1, _ = first_pair(x, d0, rnd)
    x2, _ = pair(x1, d0.conv[2], d0.conv[3], conv_w(d0.conv[2], False)[1], conv_w(d0.conv[3], False)[1], x1, rnd=rnd)
    st["d0.x1"], st["d0.x2"] = x1, x2
    feats = [x2]
    for i in range(1, len(net.down)):
        blk = net.down[i]
        xin = F.max_pool2d(feats[-1], 2, 2)
        b = [conv_w(blk.conv[k], False)[1] for k in range(4)]
        c0, _ = unit(xin, blk.conv[0], b[0], rnd=rnd)
        if i == 1:
            x1, _ = unit_proj(c0, blk.conv[1], b[1], xin, blk.proj, rnd)
        else:
            p, _ = proj(xin, blk.proj, rnd)
            x1, _ = unit(c0, blk.conv[1], b[1] + proj_params(blk.proj, rnd)[1], res=p, rnd=rnd)
        c2, _ = unit(x1, blk.conv[2], b[2], rnd=rnd)
        x2, _ = unit(c2, blk.conv[3], b[3], res=x1, rnd=rnd)
        st[f"d{i}.c0"], st[f"d{i}.x1"], st[f"d{i}.c2"], st[f"d{i}.x2"] = c0, x1, c2, x2
        feats.append(x2)
    sv, _ = style(feats[-1])
    sh = shifts_of(net, style_shifts(net, sv)[0])
    x, up = feats[-1], False
    y = None
    for i in range(len(net.up) - 1, -1, -1):
        blk = net.up[i]
        b = [conv_w(blk.conv0, False)[1]] + [conv_w(su.conv, False)[1] for su in (blk.conv1, blk.conv2, blk.conv3)]
        pl, _ = proj(x, blk.proj, rnd)
        c0s, _ = unit(x, blk.conv0, b[0], res=feats[i], in_up=up, rnd=rnd)
        x1, _ = unit(c0s, blk.conv1.conv, b[1] + proj_params(blk.proj, rnd)[1], shift=sh[(i, 1)], res=pl, res_up=up, rnd=rnd)
        c2, _ = unit(x1, blk.conv2.conv, b[2], shift=sh[(i, 2)], rnd=rnd)
        st[f"u{i}.c0s"], st[f"u{i}.x1"], st[f"u{i}.c2"] = c0s, x1, c2
        if i == 0:
            y, _ = unit_head(c2, blk.conv3.conv, b[3], x1, net.output, shift=sh[(i, 3)], rnd=rnd)
        else:
            x, _ = unit(c2, blk.conv3.conv, b[3], shift=sh[(i, 3)], res=x1, rnd=rnd)
            st[f"u{i}.x"] = x
        up = True
    return y, sv, st


def module_forward(net, x, round_weights=True):
    """`ResidualUNet.forward` in float64 on a copy of the module, conv weights rounded to bf16 (activations are not)."""
    import copy

    m = copy.deepcopy(net).to("cpu", F64).eval()
    if round_weights:
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.Conv2d):
                    mod.weight.copy_(bf16(mod.weight))
    with torch.no_grad():
        return m(x.to("cpu", F64))


# ---------------------------------------------------------------------------------------------------------- checker
def check(name, out, ref, S, m, report=None):
    """Assert |out - ref| <= ulp_bf16(ref) + (2^-10 + m * 2^-8) * S for every element, and, when m = 0, that at least 99 % of
    the elements are bit-equal.  Returns (worst normalised error, bit-equal fraction) and appends them to `report`
    (a list of (name, values)).

    The error model.  `ref` is the stage in float64 from the kernel's own recorded inputs, rounded where the design rounds.  The
    kernel differs from it in three ways only:
      * its fp32 accumulation: K <= 9 * 256 = 2304 terms summed in fp32 (MFMA 32x32x16 blocks, then the accumulator chain)
        differ from the exact sum by at most ~log2(K) * 2^-24 * S <= 2^-12.8 * S — far below the 2^-10 * S allowed;
      * the final rounding: a value that lands on the other side of a bf16 tie than the float64 one is off by one ulp of
        `ref` — the ulp_bf16(ref) term;
      * rare flips of the prologue's bf16 rounding where scale * x + shift (an fp32 fma in the kernel) sits within an fp32
        ulp of a bf16 tie: one such flip changes one term of the sum by one bf16 ulp of that input, 2^-8 of its share of
        S; a few of them in one sum stay under the 2^-10 * S left after the accumulation term;
      * every internal rounding of a partial result (the pair's intermediate, the K-split's partial sums, the first pair's
        c0, the head's input) can itself flip by one ulp, i.e. 2^-8 of the majorant of that partial result, which S
        carries forward: m * 2^-8 * S.
    The bound is derived from this model, not fitted to observed errors."""
    out = out.to(F64)
    ref = ref.to(F64)
    S = S.to(F64).expand_as(ref)
    tol = ulp_bf16(ref) + (2.0 ** -10 + m * 2.0 ** -8) * S
    err = (out - ref).abs()
    norm = torch.where(tol > 0, err / tol, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(norm.max()) if norm.numel() else 0.0
    equal = float((out == ref).to(F64).mean()) if out.numel() else 1.0
    if report is not None:
        report.append((name, dict(m=m, worst=worst, bit_equal=equal)))
    bad = norm > 1.0
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound (worst {worst:.3g} of it); "
                             f"first at {idx}: out {float(out[idx])!r} ref {float(ref[idx])!r} tol {float(tol[idx])!r}")
    if m == 0:
        assert equal >= 0.99, f"{name}: only {equal:.4f} of the elements are bit-equal to the reference"
    return worst, equal
