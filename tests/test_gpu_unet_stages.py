"""
The fused U-Net forward (aliby_amd/segment/fused_unet.py) checked launch by launch, sample by sample and element by element
against the float64 stage references of tests/unet_stage_ref.py.

Every launch helper of FusedUNet is wrapped (monkeypatch, no product change) so that the inputs and outputs of each launch
are copied to the host for the checked samples.  Then, per shape and batch size:
  * the launch sequence (helper, unit, launch form) is the one the shape calls for;
  * every stage input is bit-identical to the recorded output that the module's forward says feeds it;
  * every stage output is within the per-element bound of `unet_stage_ref.check` of its float64 reference computed from the
    recorded inputs and the module's own parameters (so wrong folded constants, halo rows, tile columns, channels or
    per-sample shifts fail here even when they move the global error by well under 1 %);
  * the style vector and the styled units' shifts match float64 values derived from the module;
  * the final output is within 2 % relative L2 of the float64 module forward per sample, no worse on the border than inside;
  * each checked sample gives the same bits when run alone.
"""

import copy
import inspect

import pytest
import torch
import torch.nn.functional as F

from tests import unet_stage_ref as sr

pytestmark = pytest.mark.gpu

HELPERS = ("_first_pair", "_unit", "_unit_proj", "_pair", "_unit_head", "_proj")


@pytest.fixture(scope="module")
def nets():
    from aliby_amd.segment.unet import build_network

    net = build_network(seed=5, device="cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    return net, copy.deepcopy(net).cpu().double()


def _tiles(n, h, w, seed):
    """Every sample different: smoothed noise with a per-sample gain and offset; sample 1 all zero (a background tile after
    normalize99), the last one bright discs on dark, the one before it with a zero second channel."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, 2, h, w, generator=g)
    for _ in range(2):
        x = F.avg_pool2d(x, 5, stride=1, padding=2, count_include_pad=False)
    x = x / x.std(dim=(2, 3), keepdim=True)
    gain = 0.2 + 2.0 * torch.rand(n, 1, 1, 1, generator=g)
    off = torch.rand(n, 2, 1, 1, generator=g) * 1.5 - 0.5
    x = x * gain + off
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    discs = torch.zeros(h, w)
    for k in range(6):
        cy, cx = float(torch.rand(1, generator=g)) * h, float(torch.rand(1, generator=g)) * w
        r = 2.0 + float(torch.rand(1, generator=g)) * max(2.0, min(h, w) / 6)
        discs = torch.where((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r, torch.full_like(discs, 0.9 + 0.1 * k / 6), discs)
    used = {0}
    for idx, kind in ((1, "zero"), (n - 1, "discs"), (n - 2, "zero_c1")):
        if idx in used or not 0 < idx < n:
            continue
        used.add(idx)
        if kind == "zero":
            x[idx] = 0.0
        elif kind == "discs":
            x[idx, 0] = discs
            x[idx, 1] = 0.3 * discs + 0.05
        else:
            x[idx, 1] = 0.0
    return x.contiguous()


class Recorder:
    """Host copies of the checked samples' slices of every launch helper's tensors, in call order."""

    def __init__(self, idx):
        self.idx = list(idx)
        self.stages = []
        self.forms = None

    def take(self, t):
        if not isinstance(t, torch.Tensor):
            return t
        if t.ndim == 1:
            return t.detach().cpu()
        return t[self.idx].detach().cpu()

    def install(self, mp, FusedUNet):
        for name in HELPERS:
            orig = getattr(FusedUNet, name)
            sig = inspect.signature(orig)

            def wrapped(fself, *a, _orig=orig, _sig=sig, _name=name, **k):
                ba = _sig.bind(fself, *a, **k)
                ba.apply_defaults()
                self.forms = []
                out = _orig(fself, *a, **k)
                args = {key: v for key, v in ba.arguments.items() if key != "self"}
                objs = {key: v for key, v in args.items() if not isinstance(v, (torch.Tensor, bool, int, type(None)))}
                rec = dict(kind=_name, objs=objs, forms=self.forms, args={key: self.take(v) for key, v in args.items()})
                if isinstance(out, tuple):
                    rec["out"], rec["pooled"] = self.take(out[0]), self.take(out[1])
                else:
                    rec["out"] = self.take(out)
                if _name == "_unit_head":
                    rec["out"] = self.take(args["y"])  # written in place
                self.stages.append(rec)
                self.forms = None
                return out

            mp.setattr(FusedUNet, name, wrapped)
        for name in ("_launch_deep", "_launch_unit"):
            orig = getattr(FusedUNet, name)

            def inner(fself, *a, _orig=orig, _name=name, **k):
                if self.forms is not None:
                    self.forms.append(("deep",) if _name == "_launch_deep" else ("slice", a[2], a[3]))  # kslice, nslice
                return _orig(fself, *a, **k)

            mp.setattr(FusedUNet, name, inner)


def _form(forms):
    """('deep' | 'single' | 'split', k-slices) of one `_unit` call's launches."""
    if forms == [("deep",)]:
        return "deep", 1
    assert forms and all(f[0] == "slice" for f in forms), forms
    nk = len({f[1] for f in forms})
    return ("single" if len(forms) == 1 else "split"), nk


def _expected_form(cin, cout, H, W, in_up, pool):
    """The launch form FusedUNet._unit is meant to choose for this shape (its docstring and the kernels' instantiations)."""
    from aliby_amd.segment.fused_unet import _MFMA_SHAPES, _POOL_SHAPES

    if cout % 128 == 0 and cin in (64, 128, 256) and W <= 56 and (H + 1) * (W + 2) >= 226 + 2 * (W + 2):
        return "deep", 1
    if (cin, cout, bool(in_up)) in (_POOL_SHAPES if pool else _MFMA_SHAPES):
        return "single", 1
    return "split", cin // (64 if cin > 64 else cin)


def _f(t):
    return None if t is None else t.to(torch.float64)


def _same(a, b, what):
    assert a is not None and b is not None and a.shape == b.shape and torch.equal(a, b), f"dataflow: {what}"


def _check_forward(case, ncpu, fused, rec, tiles, H, W, style_k, style_all_k, report):
    """Walk the recorded launches in the order of FusedUNet.__call__: launch sequence, dataflow, per-stage bounds, style."""
    it = iter(rec.stages)

    def nxt(kind, **objs):
        s = next(it, None)
        assert s is not None, f"{case}: the forward made fewer launches than expected (next: {kind})"
        assert s["kind"] == kind, f"{case}: expected {kind}, recorded {s['kind']}"
        for key, obj in objs.items():
            assert s["objs"][key] is obj, f"{case}: {kind} got the wrong {key}"
        return s

    def chk(name, s, ref_S, m):
        ref, S = ref_S
        sr.check(f"{case} {name}", _f(s["out"]), ref, S, m, report)

    def unit_stage(name, s, seq, bias, H_, W_, shift=None, res=None, res_up=False, in_up=False, pool=False):
        a = s["args"]
        x = _f(a["x"])
        cin, cout = x.shape[1], seq[-1].out_channels
        form = _form(s["forms"])
        assert form == _expected_form(cin, cout, H_, W_, in_up, pool), (case, name, form)
        chk(name, s, sr.unit(x, seq, bias, shift=shift, res=res, res_up=res_up, in_up=in_up, k_slices=form[1]), form[1] - 1)
        if pool:
            _same(_f(s["pooled"]), F.max_pool2d(_f(s["out"]), 2, 2), f"{name}: pooled output = max_pool2d(output)")
        return _f(s["out"])

    b = lambda seq: seq[-1].bias.detach().to(torch.float64)  # noqa: E731
    # ---- level 0: first layer + conv1 + projection, then conv2 + conv3 as the pair with the pooled output
    d0, f0 = ncpu.down[0], fused.down[0]
    s = nxt("_first_pair", d=f0)
    assert torch.equal(s["args"]["tiles"], tiles)
    chk("d0.first_pair", s, sr.first_pair(_f(s["args"]["tiles"]), d0), 1)
    x1 = _f(s["out"])
    s = nxt("_pair", ua=f0["u"][2], ub=f0["u"][3])
    a = s["args"]
    _same(_f(a["x"]), x1, "d0 pair input = x1")
    _same(_f(a["res"]), x1, "d0 pair residual = x1")
    assert a["pool"] and a["shift_a"] is None and a["shift_b"] is None
    chk("d0.pair", s, sr.pair(x1, d0.conv[2], d0.conv[3], b(d0.conv[2]), b(d0.conv[3]), x1), 1)
    x2 = _f(s["out"])
    _same(_f(s["pooled"]), F.max_pool2d(x2, 2, 2), "d0 pooled output = max_pool2d(x2)")
    feats, xin = [x2], _f(s["pooled"])
    h, w = H, W
    for i in range(1, 4):
        h, w = h // 2, w // 2
        blk, fd = ncpu.down[i], fused.down[i]
        p = None
        if i > 1:
            s = nxt("_proj", proj=fd["proj"])
            _same(_f(s["args"]["x"]), xin, f"d{i} projection input = pooled x2 of level {i - 1}")
            chk(f"d{i}.proj", s, sr.proj(xin, blk.proj), 0)
            p = _f(s["out"])
        s = nxt("_unit", unit=fd["u"][0])
        _same(_f(s["args"]["x"]), xin, f"d{i} conv0 input = pooled x2 of level {i - 1}")
        c0 = unit_stage(f"d{i}.c0", s, blk.conv[0], b(blk.conv[0]), h, w)
        if i == 1:
            s = nxt("_unit_proj", unit=fd["u"][1], proj=fd["proj"])
            _same(_f(s["args"]["x"]), c0, "d1 conv1 input = c0")
            _same(_f(s["args"]["x_in"]), xin, "d1 fused projection input = pooled x2 of level 0")
            chk("d1.x1", s, sr.unit_proj(c0, blk.conv[1], b(blk.conv[1]), xin, blk.proj), 0)
            x1 = _f(s["out"])
        else:
            s = nxt("_unit", unit=fd["u"][1])
            _same(_f(s["args"]["x"]), c0, f"d{i} conv1 input = c0")
            _same(_f(s["args"]["res"]), p, f"d{i} conv1 residual = projection")
            x1 = unit_stage(f"d{i}.x1", s, blk.conv[1], b(blk.conv[1]) + sr.proj_params(blk.proj, True)[1], h, w, res=p)
        s = nxt("_unit", unit=fd["u"][2])
        _same(_f(s["args"]["x"]), x1, f"d{i} conv2 input = x1")
        c2 = unit_stage(f"d{i}.c2", s, blk.conv[2], b(blk.conv[2]), h, w)
        s = nxt("_unit", unit=fd["u"][3])
        _same(_f(s["args"]["x"]), c2, f"d{i} conv3 input = c2")
        _same(_f(s["args"]["res"]), x1, f"d{i} conv3 residual = x1")
        pool = i < 3
        assert bool(s["args"]["pool"]) == pool
        x2 = unit_stage(f"d{i}.x2", s, blk.conv[3], b(blk.conv[3]), h, w, res=x1, pool=pool)
        feats.append(x2)
        xin = _f(s["pooled"]) if pool else None
    # ---- style vector and the styled units' shifts
    sv_ref, sv_mag = sr.style(feats[-1])
    sk = style_k.to(torch.float64)
    err = (sk - sv_ref).abs()
    assert bool((err <= 1e-5 * sv_ref.abs()).all()), f"{case}: style off by {float((err / sv_ref.abs()).max()):.3g} relative"
    sh_ref, sh_mag = sr.style_shifts(ncpu, sk)
    sak = style_all_k.to(torch.float64)
    assert sak.shape == sh_ref.shape
    serr = (sak - sh_ref).abs()
    assert bool((serr <= 1e-5 * sh_mag).all()), f"{case}: style shifts off by {float((serr / sh_mag).max()):.3g} of their terms"
    report.append((f"{case} style", dict(worst_of_terms=float((err / sv_mag).max()), worst_rel=float((err / sv_ref.abs()).max()))))
    report.append((f"{case} style_shifts", dict(worst_of_terms=float((serr / sh_mag).max()))))
    sh = sr.shifts_of(ncpu, sh_ref)
    # ---- up path
    x, up = feats[-1], False
    swap_stage = None
    for i in range(3, -1, -1):
        blk, fd = ncpu.up[i], fused.up[i]
        hh, ww = H >> i, W >> i
        s = nxt("_proj", proj=fd["proj"])
        _same(_f(s["args"]["x"]), x, f"u{i} projection input = the level below's output")
        chk(f"u{i}.proj", s, sr.proj(x, blk.proj), 0)
        pl = _f(s["out"])
        s = nxt("_unit", unit=fd["u"][0])
        _same(_f(s["args"]["x"]), x, f"u{i} conv0 input = the level below's output")
        _same(_f(s["args"]["res"]), feats[i], f"u{i} skip = x2 of down level {i}")
        assert bool(s["args"]["in_up"]) == up
        c0s = unit_stage(f"u{i}.c0s", s, blk.conv0, b(blk.conv0), hh, ww, res=feats[i], in_up=up)
        s = nxt("_unit", unit=fd["u"][1])
        _same(_f(s["args"]["x"]), c0s, f"u{i} conv1 input = conv0 + skip")
        _same(_f(s["args"]["res"]), pl, f"u{i} conv1 residual = projection")
        assert bool(s["args"]["res_up"]) == up
        x1 = unit_stage(f"u{i}.x1", s, blk.conv1.conv, b(blk.conv1.conv) + sr.proj_params(blk.proj, True)[1], hh, ww,
                        shift=sh[(i, 1)], res=pl, res_up=up)
        s = nxt("_unit", unit=fd["u"][2])
        _same(_f(s["args"]["x"]), x1, f"u{i} conv2 input = x1")
        c2 = unit_stage(f"u{i}.c2", s, blk.conv2.conv, b(blk.conv2.conv), hh, ww, shift=sh[(i, 2)])
        if i == 1:
            swap_stage = (s, blk.conv2.conv, b(blk.conv2.conv), x1, sh[(i, 2)])
        if i > 0:
            s = nxt("_unit", unit=fd["u"][3])
            _same(_f(s["args"]["x"]), c2, f"u{i} conv3 input = c2")
            _same(_f(s["args"]["res"]), x1, f"u{i} conv3 residual = x1")
            x = unit_stage(f"u{i}.x", s, blk.conv3.conv, b(blk.conv3.conv), hh, ww, shift=sh[(i, 3)], res=x1)
        else:
            s = nxt("_unit_head", unit=fd["u"][3])
            _same(_f(s["args"]["x"]), c2, "u0 last unit input = c2")
            _same(_f(s["args"]["res"]), x1, "u0 last unit residual = x1")
            chk("u0.x+head", s, sr.unit_head(c2, blk.conv3.conv, b(blk.conv3.conv), x1, ncpu.output, shift=sh[(0, 3)]), 1)
        up = True
    assert next(it, None) is None, f"{case}: launches after the output head"
    # ---- the inputs make the per-sample style check sensitive: swapping two samples' shifts fails the bound
    s, seq, bias, x1, shift = swap_stage
    ref, S = sr.unit(x1, seq, bias, shift=shift)
    for j in range(len(rec.idx) - 1):
        perm = list(range(len(rec.idx)))
        perm[j], perm[j + 1] = perm[j + 1], perm[j]
        bad, _ = sr.unit(x1, seq, bias, shift=shift[perm])
        with pytest.raises(AssertionError, match="outside the bound"):
            sr.check(f"{case} swapped shifts {rec.idx[j]}<->{rec.idx[j + 1]}", bad[[j, j + 1]], ref[[j, j + 1]], S[[j, j + 1]], 0)


CASES = [  # (H, W, N, checked samples or None for all)
    (224, 224, 288, (0, 1, 7, 8, 286, 287)),  # production batch: packed launches at every deep level
    (224, 224, 9, None),                      # one more than a packed group at 28 px: the plain fallback
    (256, 256, 5, None),
    (16, 16, 3, None),                        # K/N-split at the deep levels
    (32, 32, 2, None),
    (24, 40, 7, None),                        # K/N-split at the deep levels
    (176, 208, 2, None),
    (64, 96, 5, None),                        # K/N-split at level 3
]


@pytest.mark.parametrize("H,W,N,idx", CASES)
def test_fused_unet_stage_by_stage(engine, nets, monkeypatch, H, W, N, idx):
    from aliby_amd.segment.fused_unet import FusedUNet

    net, ncpu = nets
    idx = list(range(N)) if idx is None else list(idx)
    case = f"{H}x{W} N={N}"
    tiles = _tiles(N, H, W, seed=H * 1000 + W + N)
    x = tiles.cuda()
    fused = FusedUNet(net, engine)
    rec = Recorder(idx)
    with monkeypatch.context() as mp:
        rec.install(mp, FusedUNet)
        y, style = fused(x)
        torch.cuda.synchronize()
    style_all = fused._style_all[idx].cpu()
    y_sel, style_sel = y[idx].cpu(), style[idx].cpu()
    report = []
    _check_forward(case, ncpu, fused, rec, tiles[idx], H, W, style_sel, style_all, report)
    assert torch.equal(rec.stages[-1]["out"], y_sel)
    # per sample against the float64 module forward (bf16-rounded weights): global, and border strips against the interior
    y_mod, _ = sr.module_forward(ncpu, tiles[idx])
    yk = y_sel.to(torch.float64)
    inner = torch.zeros(H, W, dtype=torch.bool)
    inner[2:-2, 2:-2] = True
    for j, n in enumerate(idx):
        e = float((yk[j] - y_mod[j]).norm() / y_mod[j].norm())
        eb = float((yk[j][:, ~inner] - y_mod[j][:, ~inner]).norm() / y_mod[j][:, ~inner].norm())
        ei = float((yk[j][:, inner] - y_mod[j][:, inner]).norm() / y_mod[j][:, inner].norm())
        report.append((f"{case} y[{n}]", dict(rel_l2=e, border=eb, interior=ei)))
        assert e <= 0.02, (case, n, e)
        assert eb <= 2 * ei, (case, n, eb, ei)
    # batch invariance: each checked sample alone gives the same bits
    for j, n in enumerate(idx):
        y1, s1 = fused(x[n : n + 1].contiguous())
        assert torch.equal(y1[0].cpu(), y_sel[j]), (case, n, "y differs from the sample run alone")
        assert torch.equal(s1[0].cpu(), style_sel[j]), (case, n, "style differs from the sample run alone")
    for name, vals in report:
        print(f"{name:<36s} " + "  ".join(f"{k}={v:.4g}" for k, v in vals.items()))


def test_run_network_in_chunks_across_frames_matches_single_frames(engine):
    """Eager run_network on three frames with a batch size whose chunks straddle frames and leave a short tail gives the bits
    of three single-frame calls (the launch form depends on the batch only through packing, which does not change bits)."""
    import warnings

    from aliby_amd import synth
    from aliby_amd.segment.cellpose_hip import CellposeModel

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = CellposeModel(net_dtype="bfloat16", seed=5, batch_size=4)
    frames = [synth.make_fov(1, s, shape=(300, 420), n_target=12)["pixels"][0, 0] for s in (3, 4, 5)]
    img = torch.from_numpy(__import__("numpy").stack(frames)).cuda()
    g = model._geometry(300, 420)
    per_frame = g["ny"] * g["nx"]
    assert per_frame % 4 != 0 and (3 * per_frame) % 4 != 0, per_frame  # chunks straddle frames, the last one is short
    assert not model.use_graph
    dP, prob = model.run_network(img)
    for f in range(3):
        dPf, probf = model.run_network(img[f : f + 1], batch_size=288)
        assert torch.equal(dP[f : f + 1], dPf) and torch.equal(prob[f : f + 1], probf), f
