// conv_upmap.h — the index map of the K-loop convolutions that read their input through the nearest-neighbour 2x upsample
// (nn_conv_deep.hip, UP instantiations).  Plain integer functions without a HIP dependency, so that a host program can check
// them position by position (tests/test_cpu_conv_upmap.py compiles tests/conv_upmap_host.cpp against this file).
//
// The kernels compute on the tall zero-separated image at OUTPUT resolution (H x W per image): width LW = W + 2 (a zero column
// left and right), period HP = H + 1 rows (one shared zero row between images, one in front of the first), flattened row-major.
// The activated window lives in LDS at INPUT resolution: the same construction over the H/2 x W/2 images, width LWl = W/2 + 2,
// period HPl = H/2 + 1.  Padded column c in [0, W + 1] maps to low column (c + 1) >> 1, padded row r' in [0, H] of a period to
// low row (r' + 1) >> 1 of the low period: zero columns land on zero columns, the shared zero row on the shared zero row, and
// pixel (y, x) on pixel (y >> 1, x >> 1).  Row R of the tall image is period R / HP, r' = R % HP.
//
// An output position in column c, row y of image n (tall row 1 + n HP + y) reads the 3 x 3 positions whose first is
// (tall row n HP + y, column c - 1).  In the low image tap (dy, dx) lies up_tap() behind the low position of that first one:
// rows 0, (y + 1) & 1, 1 and columns 0, c & 1, 1 further: two of three offsets per axis are constants, the middle one is the
// parity of the position.  (This holds for every position that is stored, y < H and 1 <= c <= W; the others are computed and
// dropped, and only have to read inside the window image.)
#pragma once

#if defined(__HIPCC__)
#define UPMAP_HD __host__ __device__
#else
#define UPMAP_HD
#endif

UPMAP_HD inline int up_low_width(int LW) { return (LW >> 1) + 1; }   // LW = W + 2, W even
UPMAP_HD inline int up_low_period(int HP) { return (HP >> 1) + 1; }  // HP = H + 1, H even
// low tall row of tall row R
UPMAP_HD inline int up_low_row(int R, int HP) {
  const int n = R / HP, r = R - n * HP;
  return n * up_low_period(HP) + ((r + 1) >> 1);
}
UPMAP_HD inline int up_low_col(int c) { return (c + 1) >> 1; }
// low flat position of the first window position (row n HP + y, column c - 1) of the output position (c, y, n)
UPMAP_HD inline int up_base(int c, int y, int n, int LW, int HP) {
  return (n * up_low_period(HP) + ((y + 1) >> 1)) * up_low_width(LW) + (c >> 1);
}
UPMAP_HD inline int up_row_bit(int y) { return (y + 1) & 1; }
UPMAP_HD inline int up_col_bit(int c) { return c & 1; }
// low flat position of tap (dy, dx) in {0, 1, 2}^2 of an output position with base `base` and parity bits rbit, cbit
UPMAP_HD inline int up_tap(int base, int rbit, int cbit, int LWl, int dy, int dx) {
  return base + (dy == 0 ? 0 : dy == 1 ? rbit : 1) * LWl + (dx == 0 ? 0 : dx == 1 ? cbit : 1);
}
// The low positions [lstart, lstart + count) that cover the window of the tile of `run` output positions from q0 on, i.e. the
// tall positions q0 - LW - 1 .. q0 + run + LW.  A first (last) tall row that shares its low row with the row after (before) it
// needs that low row from its first (to its last) column; otherwise the low row starts (ends) where the window does.
// lstart = (np * HPl + rp) * LWl + cp: column cp of row rp in [0, HPl) of low period np.
UPMAP_HD inline void up_win_span(int q0, int run, int LW, int HP, int& lstart, int& count, int& np, int& rp, int& cp) {
  const int LWl = up_low_width(LW);
  const int pf = q0 - LW - 1, pl = q0 + run + LW;
  const int Rf = pf / LW, cf = pf - Rf * LW, Rl = pl / LW, cl = pl - Rl * LW;
  const int lf = up_low_row(Rf, HP), ll = up_low_row(Rl, HP);
  np = Rf / HP;
  rp = lf - np * up_low_period(HP);
  cp = up_low_row(Rf + 1, HP) == lf ? 0 : up_low_col(cf);
  lstart = lf * LWl + cp;
  count = ll * LWl + (up_low_row(Rl - 1, HP) == ll ? LWl - 1 : up_low_col(cl)) - lstart + 1;
}
UPMAP_HD inline void up_win_span(int q0, int run, int LW, int HP, int& lstart, int& count) {
  int np, rp, cp;
  up_win_span(q0, run, LW, HP, lstart, count, np, rp, cp);
}
