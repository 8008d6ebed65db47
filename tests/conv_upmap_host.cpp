// Host-side view of aliby_amd/csrc/conv_upmap.h for tests/test_cpu_conv_upmap.py: the functions the UP convolution kernels address
// their low-resolution window with, evaluated for every output position of a batch.  Compiled by the test with the host compiler.
#include "../aliby_amd/csrc/conv_upmap.h"

extern "C" {

// For every position q in [LW, N * HP * LW) of the tall output image and every tap: taps[(q - LW) * 9 + 3 dy + dx] = low flat position.
// (column, row, image) of q as the kernels derive them: r = q / LW, n = (r - 1) / HP, y = (r - 1) - n * HP.
void upmap_taps(int H, int W, int N, int* taps) {
  const int LW = W + 2, HP = H + 1, LWl = up_low_width(LW);
  for (int q = LW; q < N * HP * LW; ++q) {
    const int r = q / LW, c = q - r * LW, n = (r - 1) / HP, y = (r - 1) - n * HP;
    const int base = up_base(c, y, n, LW, HP);
    for (int dy = 0; dy < 3; ++dy)
      for (int dx = 0; dx < 3; ++dx) taps[(q - LW) * 9 + 3 * dy + dx] = up_tap(base, up_row_bit(y), up_col_bit(c), LWl, dy, dx);
  }
}

// out = {lstart, count, np, rp, cp} of the tile of `run` positions from q0 on
void upmap_span(int q0, int run, int H, int W, int* out) {
  up_win_span(q0, run, W + 2, H + 1, out[0], out[1], out[2], out[3], out[4]);
}

int upmap_low_row(int R, int H) { return up_low_row(R, H + 1); }
int upmap_low_col(int c) { return up_low_col(c); }
}
