"""
The argument checks of the engine's volume methods (intensity3d, intensity3d_detail, sizeshape3d and its surface column, coloc3d,
texture3d, neighbors3d) are host logic: every refusal here is raised before anything touches a device, so none of these tests is
marked `gpu`.  The GPU files (tests/test_gpu_*3d*.py, test_gpu_volume.py) pin the same refusals in front of a real launch.

A method is called on an engine that was never initialised (no context, no library): a refusal that came after any device work
would fail on the missing attribute instead of raising what is expected.  `_Resident` is a CPU tensor that answers `is_cuda` with
True, so that the checks behind "is it on the device" can be reached; they read shapes and dtypes only.
"""
import numpy as np
import pytest
import torch

from aliby_amd.extraction import features as feat
from aliby_amd.extraction.engine import FeatureEngine


class _Resident(torch.Tensor):
    is_cuda = True


def _resident(t: torch.Tensor) -> torch.Tensor:
    return t.as_subclass(_Resident)


F, C, Z, Y, X = 2, 2, 2, 3, 4
VOL = _resident(torch.zeros((F, Z, Y, X), dtype=torch.uint16))
PIX = _resident(torch.zeros((F, C, Z, Y, X), dtype=torch.uint16))
COUNTS = [1, 2]
ENGINE = object.__new__(FeatureEngine)  # no __init__: no device

# (method, arguments after the labels and the counts in front of them where the method takes pixels) -> a call with every argument by name
WITH_PIXELS = {
    "intensity3d": dict(channel=0),
    "intensity3d_detail": dict(channel=0),
    "coloc3d": dict(pairs=[(0, 1)]),
    "texture3d": dict(channel=0),
}
LABELS_ONLY = {"sizeshape3d": dict(), "neighbors3d": dict()}
ALL = {**WITH_PIXELS, **LABELS_ONLY}


def call(name, **kw):
    args = dict(volume=VOL, counts=COUNTS, **ALL[name])
    if name in WITH_PIXELS:
        args["pixels"] = PIX
    args.update(kw)
    return getattr(ENGINE, name)(**args)


def test_the_fixture_passes_every_check():
    """The good arguments get through all the checks and fail only where the device is first needed."""
    assert FeatureEngine._volume_labels("t", VOL) == (F, Z, Y, X)
    got = FeatureEngine._volume_inputs("t", VOL, PIX, COUNTS)
    assert got[:5] == (F, C, Z, Y, X) and got[5].dtype == np.int32 and got[5].tolist() == [0, 1, 3]
    for name in ALL:
        with pytest.raises(AttributeError):  # the uninitialised engine has no device to allocate the result on
            call(name)


@pytest.mark.parametrize("name", sorted(ALL))
def test_labels(name):
    with pytest.raises(TypeError, match="torch tensors"):
        call(name, volume=VOL.numpy())
    for dtype in (torch.int32, torch.int16, torch.float32):
        with pytest.raises(TypeError, match="must be uint16"):
            call(name, volume=_resident(torch.zeros((F, Z, Y, X), dtype=dtype)))
    for shape in ((Z, Y, X), (F, 1, Z, Y, X)):
        with pytest.raises(ValueError, match=r"\[F,Z,Y,X\]"):
            call(name, volume=_resident(torch.zeros(shape, dtype=torch.uint16)))
    with pytest.raises(ValueError, match="on the device"):
        call(name, volume=torch.zeros((F, Z, Y, X), dtype=torch.uint16))


@pytest.mark.parametrize("name", sorted(WITH_PIXELS))
def test_pixels(name):
    with pytest.raises(TypeError, match="torch tensors"):
        call(name, pixels=PIX.numpy())
    for dtype in (torch.float64, torch.int16, torch.int32, torch.uint8):
        with pytest.raises(TypeError, match="pixels must be uint16"):
            call(name, pixels=_resident(torch.zeros((F, C, Z, Y, X), dtype=dtype)))
    # rank 4, rank 6, and another F, Z, Y or X than the labels'
    for shape in ((F, Z, Y, X), (F, C, 1, Z, Y, X), (F + 1, C, Z, Y, X), (F, C, Z + 1, Y, X), (F, C, Z, Y - 1, X), (F, C, Z, Y, X + 1)):
        with pytest.raises(ValueError, match=r"pixels \[F,C,Z,Y,X\]"):
            call(name, pixels=_resident(torch.zeros(shape, dtype=torch.uint16)))
    with pytest.raises(ValueError, match="on the device"):
        call(name, pixels=torch.zeros((F, C, Z, Y, X), dtype=torch.uint16))
    # a TypeError of the pixels or the labels comes before any ValueError
    with pytest.raises(TypeError):
        call(name, volume=_resident(torch.zeros((Z, Y, X), dtype=torch.uint16)), pixels=_resident(torch.zeros((F, C, Z, Y, X), dtype=torch.float64)))
    with pytest.raises(TypeError):
        call(name, volume=_resident(torch.zeros((F, Z, Y, X), dtype=torch.int32)), pixels=_resident(torch.zeros((F, Z, Y, X), dtype=torch.uint16)))


def test_intensity3d_has_no_float_form():
    with pytest.raises(TypeError, match="no float form"):
        call("intensity3d", pixels=_resident(torch.zeros((F, C, Z, Y, X), dtype=torch.float32)))
    for name in ("intensity3d_detail", "coloc3d", "texture3d"):
        with pytest.raises(AttributeError):  # float32 pixels pass the checks
            call(name, pixels=_resident(torch.zeros((F, C, Z, Y, X), dtype=torch.float32)))


@pytest.mark.parametrize("name", sorted(ALL))
def test_counts(name):
    for bad in ([1], [1, 2, 3], [[1, 2], [3, 4]], [1, -1], [65536, 0], []):
        with pytest.raises(ValueError, match="counts must hold one label count"):
            call(name, counts=bad)
    assert FeatureEngine._volume_offsets("t", 2, [65535, 0]).tolist() == [0, 65535, 65535]
    assert FeatureEngine._volume_offsets("t", 3, np.asarray([0, 0, 0], np.uint8)).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["intensity3d", "intensity3d_detail", "texture3d"])
def test_channel(name):
    for bad in (True, False, 0.0, 1.5, "0", None):
        with pytest.raises(TypeError, match="channel must be an integer"):
            call(name, channel=bad)
    for bad in (C, -1, np.int64(C)):
        with pytest.raises(ValueError, match=f"out of range for {C} channels"):
            call(name, channel=bad)
    with pytest.raises(AttributeError):  # a NumPy integer in range is a channel
        call(name, channel=np.int32(C - 1))
    assert FeatureEngine._channel(np.uint8(1), 2) == 1 and type(FeatureEngine._channel(np.uint8(1), 2)) is int


def test_intensity3d_detail_flag_comes_before_the_channel_range():
    for flag in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="edge_measurements must be a bool"):
            call("intensity3d_detail", channel=C, edge_measurements=flag)


def test_texture3d_parameters():
    for kw in (dict(scale=1.5), dict(scale=True), dict(gray_levels=256.0), dict(gray_levels="256")):
        with pytest.raises(TypeError, match="must be an integer"):
            call("texture3d", **kw)
        with pytest.raises(TypeError):  # ... and before the range of the channel
            call("texture3d", channel=C, **kw)
    for kw in (dict(scale=0), dict(gray_levels=1), dict(gray_levels=257)):
        with pytest.raises(ValueError, match="texture3d needs scale >= 1"):
            call("texture3d", **kw)


def test_coloc3d_parameters():
    for kw in (dict(pairs=[]), dict(pairs=[(0, 1)] * 65), dict(pairs=[(0, C)]), dict(pairs=[(0, 0)]), dict(pairs=[(0, 1, 2)]), dict(metrics=()),
               dict(metrics=("pearson", "pearson")), dict(metrics=("spearman",)), dict(thr=float("nan")), dict(scale_max=0.0), dict(scale_max=float("inf"))):
        with pytest.raises(ValueError):
            call("coloc3d", **kw)


def test_spacing_and_the_surface_column():
    for bad in ((1.0, 1.0, 0.0), (1.0, -1.0, 1.0), (float("nan"), 1.0, 1.0), (float("inf"), 1.0, 1.0)):
        with pytest.raises(ValueError, match="three positive finite numbers"):
            call("sizeshape3d", spacing=bad)
        with pytest.raises(ValueError, match="three positive finite numbers"):
            FeatureEngine.surface3d_table(bad)
    for bad in ((1.0, 1.0), (1.0, 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            call("sizeshape3d", spacing=bad)
    assert FeatureEngine._spacing3d([0.5, 1, 2]).tolist() == [0.5, 1.0, 2.0]
    thin = _resident(torch.zeros((F, 1, Y, X), dtype=torch.uint16))
    with pytest.raises(ValueError, match="at least 2 x 2 x 2"):
        call("sizeshape3d", volume=thin, surface_area=True)
    with pytest.raises(AttributeError):  # without the column one plane is a volume
        call("sizeshape3d", volume=thin)
    # the labels are looked at first, the counts last
    with pytest.raises(TypeError):
        call("sizeshape3d", volume=VOL.numpy(), spacing=(0, 0, 0), counts=[1])
    with pytest.raises(ValueError, match="three positive finite numbers"):
        call("sizeshape3d", spacing=(0, 0, 0), counts=[1])


@pytest.mark.parametrize("distance_of, cap, family", [(feat.neighbors_distance, feat.NEIGHBORS_MAX_DISTANCE, "neighbors"),
                                                      (feat.neighbors3d_distance, feat.NEIGHBORS3D_MAX_DISTANCE, "neighbors3d")])
def test_neighbour_distances(distance_of, cap, family):
    assert (feat.NEIGHBORS_MAX_DISTANCE, feat.NEIGHBORS3D_MAX_DISTANCE) == (64, 16)
    assert distance_of() == distance_of(None) == 1
    for d in (1, 2, cap, np.int16(cap), np.uint8(3)):
        assert distance_of(d) == int(d) and type(distance_of(d)) is int
    for bad in (0, -1, cap + 1, 2.5, 1.0, True, False, "3", [3]):
        with pytest.raises(ValueError, match=rf"^{family}: distance must be None or an integer in 1\.\.{cap}, got "):
            distance_of(bad)


def test_neighbors3d_checks_the_distance_first():
    for bad in (0, 17, 2.5, True, "3"):
        with pytest.raises(ValueError, match="neighbors3d: distance"):
            call("neighbors3d", distance=bad)
        with pytest.raises(ValueError, match="neighbors3d: distance"):  # ... before the labels' TypeError
            call("neighbors3d", volume=VOL.numpy(), distance=bad)
    with pytest.raises(AttributeError):
        call("neighbors3d", distance=16)


def test_neighbour_names_share_their_stems():
    stems = ["NumberOfNeighbors", "PercentTouching", "FirstClosestObjectNumber", "FirstClosestDistance", "SecondClosestObjectNumber",
             "SecondClosestDistance", "AngleBetweenNeighbors"]
    for names_of, cap in ((feat.neighbors_names, 64), (feat.neighbors3d_names, 16)):
        assert names_of() == names_of(None) == [f"Neighbors_{s}_Adjacent" for s in stems]
        for d in (1, 5, cap):
            assert names_of(d) == [f"Neighbors_{s}_{d}" for s in stems]
        with pytest.raises(ValueError):
            names_of(cap + 1)
    assert feat.neighbors_names(16) == feat.neighbors3d_names(16)
    assert feat.neighbors_names(17)[0] == "Neighbors_NumberOfNeighbors_17"
    assert feat.family_names("neighbors", distance=3) == feat.neighbors_names(3)
