"""
The index map of the convolutions that keep their window at input resolution and read it through the 2x upsample
(aliby_amd/csrc/conv_upmap.h, used by the UP kernels of nn_conv_deep.hip), checked on the CPU: the header is plain integer code,
compiled here with the host compiler (tests/conv_upmap_host.cpp) and called through ctypes.

For every output position and tap of H, W in {28, 56, 112} and N <= 3 the map names the pixel that upsample -> zero-pad puts
there, or a position of the zero row / column; the low window of every tile holds every tap of the positions the tile stores,
starts where its (period, row, column) form says, and fits the planes the kernels allocate.
"""

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def upmap(tmp_path_factory):
    so = tmp_path_factory.mktemp("upmap") / "libupmap.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", str(ROOT / "tests" / "conv_upmap_host.cpp"), "-o", str(so)],
                   check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    lib.upmap_taps.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.upmap_span.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    return lib


def _tall(ids):
    """[N, h, w] ids (> 0) -> the tall zero-separated image: a zero row, then per image h rows and a zero row; a zero column each side."""
    n, h, w = ids.shape
    t = np.zeros((n * (h + 1) + 1, w + 2), dtype=np.int64)
    for i in range(n):
        t[1 + i * (h + 1):1 + i * (h + 1) + h, 1:w + 1] = ids[i]
    return t


def _taps(upmap, H, W, N):
    LW, HP = W + 2, H + 1
    taps = np.zeros(((N * HP - 1) * LW, 9), dtype=np.int32)
    upmap.upmap_taps(H, W, N, taps.ctypes.data)
    return taps


SHAPES = [(H, W, N) for H in (28, 56, 112) for W in (28, 56, 112) for N in (1, 2, 3)]


@pytest.mark.parametrize("H,W,N", SHAPES)
def test_every_tap_of_every_position_is_the_pixel_upsample_then_pad_puts_there(upmap, H, W, N):
    LW, HP = W + 2, H + 1
    ids = 1 + np.arange(N * (H // 2) * (W // 2), dtype=np.int64).reshape(N, H // 2, W // 2)
    low = _tall(ids).ravel()
    high = _tall(ids.repeat(2, axis=1).repeat(2, axis=2))  # upsample, then pad
    taps = _taps(upmap, H, W, N)
    q = np.arange(LW, N * HP * LW)
    r, c = q // LW, q % LW
    stored = ((r - 1) % HP < H) & (c >= 1) & (c <= W)
    assert stored.sum() == N * H * W
    hf = high.ravel()
    for dy in range(3):
        for dx in range(3):
            want = hf[q[stored] + (dy - 1) * LW + (dx - 1)]
            got = low[taps[stored, 3 * dy + dx]]
            assert np.array_equal(got, want), (dy, dx)
    # the zero row and the zero columns are hit exactly where the padding is
    assert (low[taps[stored]] == 0).sum() == (hf[q[stored][:, None] + np.array([(dy - 1) * LW + dx - 1 for dy in range(3) for dx in range(3)])] == 0).sum()


def _const(name):
    src = (ROOT / "aliby_amd" / "csrc" / "nn_conv_deep.hip").read_text()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


@pytest.mark.parametrize("run,cap_name,shapes", [
    (224, "DCU_WIN_MAX", [(28, 28), (56, 56), (28, 56), (56, 28), (2, 2), (6, 54), (30, 20)]),
    (448, "UU_WIN_MAX", [(112, 112), (128, 128), (56, 112), (28, 28), (2, 4), (8, 126)]),
])
def test_the_low_window_of_every_tile_holds_its_taps_and_fits_the_planes(upmap, run, cap_name, shapes):
    cap = _const(cap_name)
    for H, W in shapes:
        for N in (1, 3, 8):
            LW, HP = W + 2, H + 1
            LWl, HPl = W // 2 + 2, H // 2 + 1
            taps = _taps(upmap, H, W, N)
            q = np.arange(LW, N * HP * LW)
            stored = ((q // LW - 1) % HP < H) & (q % LW >= 1) & (q % LW <= W)
            out = np.zeros(5, dtype=np.int32)
            for q0 in range(LW, N * HP * LW, run):
                upmap.upmap_span(q0, run, H, W, out.ctypes.data)
                lstart, count, np_, rp, cp = (int(v) for v in out)
                assert 0 < count <= cap, (H, W, N, q0, count)
                assert lstart == (np_ * HPl + rp) * LWl + cp and 0 <= rp < HPl and 0 <= cp < LWl
                sel = slice(q0 - LW, min(q0 + run, N * HP * LW) - LW)
                t = taps[sel][stored[sel]]
                if t.size:
                    assert lstart <= t.min() and t.max() < lstart + count, (H, W, N, q0)
                    # and the clamp of the lane bases (plane - LWl - 2 with plane >= cap) never moves a stored position
                    assert t[:, 0].max() - lstart <= cap - LWl - 2


def test_rows_and_columns_map_as_the_header_says(upmap):
    for H in (2, 28, 56):
        lows = [upmap.upmap_low_row(R, H) for R in range(3 * (H + 1) + 1)]
        assert lows[0] == 0 and lows[1] == 1
        for n in range(3):  # zero rows land on zero rows, pixel row y on pixel row y >> 1
            assert lows[n * (H + 1)] == n * (H // 2 + 1)
            assert [lows[n * (H + 1) + 1 + y] for y in range(H)] == [n * (H // 2 + 1) + 1 + (y >> 1) for y in range(H)]
    assert [upmap.upmap_low_col(c) for c in range(8)] == [0, 1, 1, 2, 2, 3, 3, 4]
