"""
csrc/objects.hip through the C ABI and engine.object_table: aliby_label_max, aliby_object_table and aliby_relabel_sequential
against tests/stager_ref.object_rows and oracle/tiler_ref.relabel_sequential, at shapes that reach the second pass of every
grid-stride loop, the vector / tail / unaligned branches of the two label readers, several frames per call and table sizes on
both sides of the true label maxima.
"""

import numpy as np
import pytest

from tests import stager_ref

pytestmark = pytest.mark.gpu


def label_max(engine, dev):
    from aliby_amd import _lib
    from aliby_amd.extraction.engine import _ptr, _stream_ptr

    F, Y, X = dev.shape
    mx = np.full(F, -7, np.int32)
    _lib.check(engine.lib.aliby_label_max(engine.ctx.handle, _ptr(dev), F, Y, X, _ptr(mx), _stream_ptr()))
    return mx.tolist()


def device_labels(labels, unaligned=False):
    import torch

    labels = np.ascontiguousarray(labels, dtype=np.uint16)
    if not unaligned:
        return torch.from_numpy(labels).cuda()
    flat = torch.zeros(labels.size + 1, dtype=torch.uint16, device="cuda")
    view = flat[1:].view(labels.shape)
    view.copy_(torch.from_numpy(labels))
    assert view.data_ptr() % 16 == 2
    return view


# ---------------------------------------------------------------------------------------------------------------- label_max
def placements(plane, aligned):
    """Pixel indices at which a lone label can be lost: first, last, inside the plane % 8 tail, last of the vector part, first
    of the second grid pass, inside the second pass.  One pass is 64 blocks x 256 lanes x 8 pixels = 131 072 on the vector path
    and 64 x 256 = 16 384 pixels on the scalar fallback of a frame whose base is not 16-byte aligned."""
    per_pass = 131072 if aligned else 16384
    nvec8 = plane // 8 * 8
    pos = {"first": 0, "last": plane - 1, "vector_end": nvec8 - 1, "pass2_first": per_pass, "pass2_inside": per_pass + 1000}
    if plane % 8:
        pos["tail"] = nvec8 + (plane % 8) // 2
    assert all(0 <= p < plane for p in pos.values())
    return pos


@pytest.mark.parametrize("F,Y,X", [(1, 368, 368), (3, 363, 373)])
@pytest.mark.parametrize("value", [1, 65535])
def test_label_max_finds_a_lone_pixel_anywhere(engine, F, Y, X, value):
    """368 x 368 = 135 424 pixels > 131 072: the vector loop's second pass (no tail: the plane is a multiple of 8).  363 x 373 =
    135 399 is odd, so frame 0 takes the vector loop plus a 7-pixel tail and frames 1 and 2 start off 16-byte alignment: the
    scalar fallback, 16 384 pixels per pass.  One nonzero pixel per call; the other frames must stay 0."""
    import torch

    plane = Y * X
    dev = torch.zeros((F, Y, X), dtype=torch.uint16, device="cuda")
    poke = dev.view(torch.int16).view(-1)  # (same bits: 65535 is -1)
    assert label_max(engine, dev) == [0] * F
    for f in range(F):
        aligned = (dev.data_ptr() + 2 * f * plane) % 16 == 0
        assert aligned == (f == 0)
        for name, p in placements(plane, aligned).items():
            poke[f * plane + p] = value if value < 32768 else value - 65536
            want = [0] * F
            want[f] = value
            assert label_max(engine, dev) == want, (f, name, p)
            poke[f * plane + p] = 0


def test_label_max_small_and_unaligned_frames(engine):
    """Frames shorter than one 16-byte group (nvec == 0: 1 x 1, 1 x 7, 3 x 3 with its second and third frame unaligned) and a
    view whose data pointer is 2-byte aligned."""
    rng = np.random.default_rng(51)
    for shape in ((1, 1, 1), (2, 1, 7), (3, 3, 3)):
        lab = rng.integers(1, 65536, size=shape).astype(np.uint16)
        assert label_max(engine, device_labels(lab)) == lab.reshape(shape[0], -1).max(axis=1).tolist()
        assert label_max(engine, device_labels(np.zeros(shape))) == [0] * shape[0]
    lab = rng.integers(0, 300, size=(2, 40, 50)).astype(np.uint16)
    lab[1, 39, 49] = 65535
    for unaligned in (False, True):
        assert label_max(engine, device_labels(lab, unaligned)) == [299, 65535]


# ------------------------------------------------------------------------------------------------------------- object table
def assert_table(table, labels, max_labels=None):
    """Every field of every row of an engine.object_table result against stager_ref.object_rows; the device copy is the host
    copy byte for byte."""
    want, offsets = stager_ref.object_rows(labels, max_labels)
    assert table.n_obj == len(want) and np.array_equal(table.offsets, offsets)
    got = table.host
    assert len(got) == len(want)
    for k in ("tile", "label", "area"):
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:5].tolist())
    present = want["area"] > 0
    for k in ("y0", "x0", "y1", "x1"):
        assert np.array_equal(got[k][present], want[k][present]), (k, np.flatnonzero((got[k] != want[k]) & present)[:5].tolist())
    assert (got["y0"][~present] > got["y1"][~present]).all()  # include/aliby_hip.h: y0 > y1 when the label is absent
    assert (got["pad_"] == 0).all()
    if table.n_obj:
        assert table.dev[: 32 * table.n_obj].cpu().numpy().tobytes() == got.tobytes()
    return want


def geometry_frame(X):
    """Rows of width X: a label that changes at every pixel; runs that start on every offset s and end on every offset e of an
    8-pixel chunk, at the left edge and in the last whole chunks of the row; a run across the whole row; and an object whose only
    pixel is the frame's last."""
    far = max(0, (X - 17) // 8 * 8)
    rows = [1 + np.arange(X) % 5]
    for base in (0, far):
        for s in range(8):
            for e in range(8):
                row = np.zeros(X, np.int64)
                row[base + s:base + 8 + e + 1] = 6 + (s * 8 + e) % 7
                rows.append(row)
    rows.append(np.full(X, 2))
    rows.append(np.zeros(X, np.int64))
    lab = np.stack(rows).astype(np.uint16)
    lab[-1, -1] = 14
    return lab


@pytest.mark.parametrize("X", [1, 7, 8, 9, 2061])
def test_object_table_run_geometry(engine, X):
    """k_table_fill reads 8-pixel chunks: rows narrower than a chunk (1, 7), exactly one (8), one and a tail (9), and 2061 — 258
    chunks, so three 128-thread blocks per row, and odd, so every second row base is off 16-byte alignment and takes the scalar
    loads while the others take the vector ones."""
    lab = geometry_frame(X)
    table = engine.object_table(device_labels(lab[None]))
    want = assert_table(table, lab[None])
    assert want["area"][13] == 1 and (want["y0"][13], want["x0"][13]) == (lab.shape[0] - 1, X - 1)
    assert want["area"][1] >= X  # the run across the whole row


def blocky(rng, shape, n_labels):
    small = rng.integers(0, n_labels + 1, size=((shape[0] + 3) // 4, (shape[1] + 3) // 4))
    return np.kron(small, np.ones((4, 4), np.int64))[: shape[0], : shape[1]].astype(np.uint16)


def four_frames():
    rng = np.random.default_rng(52)
    lab = np.zeros((4, 37, 53), np.uint16)
    lab[0] = blocky(rng, (37, 53), 11)
    lab[0][lab[0] == 4] = 0  # a gap
    lab[2] = blocky(rng, (37, 53), 23)
    lab[3, 36, 52] = 3  # one pixel: rows 1 and 2 of that frame are absent
    return lab


def test_object_table_several_frames(engine):
    """F = 4: populated, all zero (nmax == 0 between two populated frames), populated, one pixel.  The offsets arithmetic puts
    every row of every frame at its place; odd 37 x 53 planes put frames 1 and 3 off alignment."""
    lab = four_frames()
    table = engine.object_table(device_labels(lab))
    want = assert_table(table, lab)
    assert table.offsets.tolist() == [0, int(lab[0].max()), int(lab[0].max()), int(lab[0].max()) + int(lab[2].max()), len(want)]
    assert want[-3:]["area"].tolist() == [0, 0, 1]


def test_object_table_max_labels_above_below_and_zero(engine):
    """max_labels above the true maxima adds empty rows; below them, the pixels of the labels above are counted nowhere; zero
    for a populated frame gives that frame no rows.  (Equal to the true maxima: tests/test_gpu_segment.py.)"""
    lab = four_frames()
    dev = device_labels(lab)
    true_max = [int(l.max()) for l in lab]
    own = engine.object_table(dev)
    above = [m + 3 for m in true_max]
    t = engine.object_table(dev, max_labels=above)
    assert_table(t, lab, above)
    for f in range(4):
        rows, own_rows = t.host[t.offsets[f]:t.offsets[f + 1]], own.host[own.offsets[f]:own.offsets[f + 1]]
        for k in ("label", "y0", "x0", "y1", "x1", "area"):
            assert np.array_equal(rows[k][: true_max[f]], own_rows[k]), (f, k)
        assert len(rows) == true_max[f] + 3 and (rows["area"][true_max[f]:] == 0).all()
    below = [max(m - 4, 0) for m in true_max]
    t = engine.object_table(dev, max_labels=below)
    want = assert_table(t, lab, below)
    assert int(want["area"].sum()) == sum(int(((lab[f] > 0) & (lab[f] <= below[f])).sum()) for f in range(4))
    zero = [0, 0, true_max[2], 0]
    t = engine.object_table(dev, max_labels=zero)
    assert_table(t, lab, zero)
    assert t.n_obj == true_max[2] and (t.host["tile"] == 2).all()
    assert engine.object_table(dev, max_labels=[0, 0, 0, 0]).n_obj == 0


def test_object_table_row_stride(engine):
    """Labels 1, 4097 and 5000 in one 64 x 64 frame: 5 000 rows > the 4 096 one pass of k_table_init covers (16 blocks x 256);
    the rows past it still get their own tile / label and an empty box."""
    lab = np.zeros((1, 64, 64), np.uint16)
    lab[0, 3:9, 5:20] = 1
    lab[0, 30:31, 0:64] = 4097
    lab[0, 63, 63] = 5000
    table = engine.object_table(device_labels(lab))
    want = assert_table(table, lab)
    assert table.n_obj == 5000 and table.host["label"].tolist() == list(range(1, 5001))
    assert np.flatnonzero(want["area"]).tolist() == [0, 4096, 4999] and want["area"][[0, 4096, 4999]].tolist() == [90, 64, 1]


# --------------------------------------------------------------------------------------------------------- relabel_sequential
def sparse_frames():
    """F = 3 of 368 x 368 = 135 424 pixels > the 65 536 one pass of k_mark_present / k_apply_map covers (256 blocks x 256):
    disjoint label sets with 1, 65535 and gaps; in every frame one label lives only at the first pixel of the second pass and
    one only at the last pixel."""
    rng = np.random.default_rng(53)
    sets = [[1, 5, 6, 300, 65535], [2, 7, 40000, 65534], [3] + list(range(1000, 1040, 3)) + [65533]]
    lab = np.zeros((3, 368, 368), np.uint16)
    for f, s in enumerate(sets):
        flat = lab[f].reshape(-1)
        common = np.array(s[1:-1], np.uint16)
        where = rng.choice(flat.size, 4000, replace=False)
        flat[where] = common[rng.integers(0, len(common), 4000)]
        flat[65536] = s[0]
        flat[-1] = s[-1]
        assert sorted(set(flat.tolist()) - {0}) == sorted(s)
    return lab


def relabel(engine, lab):
    from oracle import tiler_ref

    dev = device_labels(lab.copy())
    n = engine.relabel_sequential(dev)
    got = dev.cpu().numpy()
    for f in range(lab.shape[0]):
        want = tiler_ref.relabel_sequential(lab[f])
        assert np.array_equal(got[f], want), (f, np.argwhere(got[f] != want)[:4].tolist())
        assert n[f] == want.max() == len(np.unique(lab[f][lab[f] > 0]))
    return n.tolist()


def test_relabel_sequential_sparse_frames_then_another_layout(engine):
    """The second call has another F right behind the first: the scratch block (presence flags | maps | counts) is cut up
    differently, and what the first call left in it must not show — an all-zero frame comes back all zero."""
    lab = sparse_frames()
    assert relabel(engine, lab) == [5, 4, 16]
    second = np.stack([np.zeros((368, 368), np.uint16), lab[2][::-1].copy()])
    assert relabel(engine, second) == [0, 16]
    assert relabel(engine, lab[1:2]) == [4]


def test_relabel_sequential_full_label_range(engine):
    """256 x 256 holding each of 1..65534 once and two zeros: the identity, n = 65534, the largest count that passes.  With
    1..65535 the count reaches 65535: the overflow error of include/aliby_hip.h (dispatch.py's uint16 guard)."""
    rng = np.random.default_rng(54)
    values = np.concatenate([np.arange(1, 65535), [0, 0]]).astype(np.uint16)
    lab = rng.permutation(values).reshape(1, 256, 256)
    dev = device_labels(lab.copy())
    assert engine.relabel_sequential(dev).tolist() == [65534]
    assert np.array_equal(dev.cpu().numpy(), lab)
    values = np.concatenate([np.arange(1, 65536), [0]]).astype(np.uint16)
    lab = rng.permutation(values).reshape(1, 256, 256)
    with pytest.raises(OverflowError, match="Segmentation produced 65535 labels; uint16 cast unsafe"):
        engine.relabel_sequential(device_labels(lab.copy()))
