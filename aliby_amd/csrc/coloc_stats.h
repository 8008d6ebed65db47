// coloc_stats.h — the per-object colocalisation statistics of one channel pair, shared by the 2-D per-pair kernel
// (feat_coloc.hip, k_coloc) and the volume kernel (feat_coloc3d.hip): everything after the gather.  The caller has the
// object's values of both channels in two float lists (LDS or global scratch, raster order); every statistic is an fp64 block
// reduction over them (block_sum_vec_all: fixed tree inside a wave, waves folded in order), so for a given workgroup size the
// result depends on the lists only.  Definitions: the header of feat_coloc.hip.
//
// `Ranks` supplies what RWC needs and nothing else touches: diff(j) = |rank1 - rank2| of element j (dense ranks inside the
// object) and R() = largest rank of either channel + 1.  The 2-D kernel reads both from its rank planes, the volume kernel
// looks them up in the object's sorted distinct values.
#pragma once
#include "common.h"

#ifdef __HIPCC__

// next probe of CellProfiler's "faster" Costes search: floor((right - left) / 1.2) + left while the bracket is wider than 6,
// else the midpoint.  The bounds are integers whenever scale_max is (left = 1, +-1 steps): floor(x / (6.0 / 5.0)) == (5 x) / 6
// and floor(x / 2.0) == x / 2 for every integer 0 <= x < 2^20 (checked exhaustively in tests/test_oracle_golden.py), which
// replaces an fp64 division per probe by integer arithmetic.
__device__ __forceinline__ double costes_next_mid(double left, double right, bool int_bounds) {
  if (int_bounds) {
    const int span = (int)(right - left);
    return (double)(span > 6 ? (5 * span) / 6 : span / 2) + left;
  }
  if (right - left > 6) return floor((right - left) / (6.0 / 5.0)) + left;
  return floor((right - left) / 2.0) + left;
}

// All threads of the workgroup call it (it contains barriers).  col_* = first of the metric's two columns in out[], -1 = not
// requested.  vec: LDS double[32], red_f: LDS float[8], red_i: LDS int[8].
template <typename Ranks>
__device__ __forceinline__ void coloc_block_stats(const float* fv, const float* sv, const int N, double* out, const int col_pearson,
                                                  const int col_manders, const int col_rwc, const int col_costes, const double thr,
                                                  const double scale_max, const Ranks& rk, double* vec, float* red_f, int* red_i) {
  const int tid = threadIdx.x;
  const double dN = (double)N;

  // ---- sums, maxima -------------------------------------------------------------------------
  double acc[8];
  float m1 = -INFINITY, m2 = -INFINITY;
  acc[0] = acc[1] = 0;
  for (int j = tid; j < N; j += blockDim.x) {
    acc[0] += (double)fv[j]; acc[1] += (double)sv[j];
    m1 = fmaxf(m1, fv[j]); m2 = fmaxf(m2, sv[j]);
  }
  double s2[2] = {acc[0], acc[1]};
  block_sum_vec_all<2>(s2, vec);
  const double mean1 = s2[0] / dN, mean2 = s2[1] / dN;
  const float MAX1 = block_max_f32(m1, red_f), MAX2 = block_max_f32(m2, red_f);

  if (col_pearson >= 0) {
    double q[3] = {0, 0, 0};
    for (int j = tid; j < N; j += blockDim.x) {
      const double x = (double)fv[j] - mean1, y = (double)sv[j] - mean2;
      q[0] += x * x; q[1] += y * y; q[2] += x * y;
    }
    block_sum_vec_all<3>(q, vec);
    if (tid == 0) {
      out[col_pearson] = q[2] / (sqrt(q[0]) * sqrt(q[1]));
      out[col_pearson + 1] = q[2] / q[0];
    }
  }

  // ---- Manders / RWC share thresholds and denominators ---------------------------------------
  const double tff = (thr / 100.0) * (double)MAX1, tss = (thr / 100.0) * (double)MAX2;
  double tot1 = 0, tot2 = 0;
  int any_comb = 0;
  if (col_manders >= 0 || col_rwc >= 0) {
    double q[4] = {0, 0, 0, 0};
    int anyc = 0;
    for (int j = tid; j < N; j += blockDim.x) {
      const double f = fv[j], s = sv[j];
      const bool a1 = f >= tff, a2 = s >= tss;
      if (a1) q[0] += f;
      if (a2) q[1] += s;
      if (a1 && a2) { q[2] += f; q[3] += s; anyc = 1; }
    }
    block_sum_vec_all<4>(q, vec);
    any_comb = block_max_i32(anyc, red_i);
    tot1 = q[0]; tot2 = q[1];
    if (col_manders >= 0 && tid == 0) {
      out[col_manders] = any_comb ? q[2] / tot1 : 0.0;
      out[col_manders + 1] = any_comb ? q[3] / tot2 : 0.0;
    }
  }

  if (col_rwc >= 0) {
    const double R = rk.R();
    double q[2] = {0, 0};
    for (int j = tid; j < N; j += blockDim.x) {
      const double f = fv[j], s = sv[j];
      if (f >= tff && s >= tss) {
        const long long di = rk.diff(j);
        const double wgt = (R - (double)di) * 1.0 / R;
        q[0] += f * wgt; q[1] += s * wgt;
      }
    }
    block_sum_vec_all<2>(q, vec);
    if (tid == 0) {
      out[col_rwc] = any_comb ? q[0] / tot1 : 0.0;
      out[col_rwc + 1] = any_comb ? q[1] / tot2 : 0.0;
    }
  }

  if (col_costes >= 0) {
    // regression line through the non-zero pixels
    double q[3] = {0, 0, 0};
    for (int j = tid; j < N; j += blockDim.x) {
      const double f = fv[j], s = sv[j];
      if (f > 0 || s > 0) { q[0] += 1; q[1] += f; q[2] += s; }
    }
    block_sum_vec_all<3>(q, vec);
    const double nnz = q[0], xmean = q[1] / nnz, ymean = q[2] / nnz, zmean = (q[1] + q[2]) / nnz;
    double v3[3] = {0, 0, 0};
    for (int j = tid; j < N; j += blockDim.x) {
      const double f = fv[j], s = sv[j];
      if (f > 0 || s > 0) {
        const double dx = f - xmean, dy = s - ymean, dz = (f + s) - zmean;
        v3[0] += dx * dx; v3[1] += dy * dy; v3[2] += dz * dz;
      }
    }
    block_sum_vec_all<3>(v3, vec);
    const double xvar = v3[0] / (nnz - 1), yvar = v3[1] / (nnz - 1), zvar = v3[2] / (nnz - 1);
    const double covar = 0.5 * (zvar - (xvar + yvar));
    const double denom = 2 * covar;
    const double num = (yvar - xvar) + sqrt((yvar - xvar) * (yvar - xvar) + 4 * (covar * covar));
    const double ca = num / denom, cb = ymean - ca * xmean;
    double left = 1, right = scale_max;
    const bool int_bounds = scale_max == floor(scale_max) && scale_max >= 1 && scale_max <= 1048576.0;
    double mid = floor((right - left) / (6.0 / 5.0)) + left;
    double lastmid = 0, valid = 1;
    for (int it = 0; it < 200 && lastmid != mid; ++it) {
      const double t1 = mid / scale_max, t2 = ca * t1 + cb;
      double c3[3] = {0, 0, 0};
      for (int j = tid; j < N; j += blockDim.x) {
        const double f = fv[j], s = sv[j];
        if (f < t1 || s < t2) { c3[0] += 1; c3[1] += f; c3[2] += s; }
      }
      block_sum_vec_all<3>(c3, vec);
      if (c3[0] <= 2) {
        left = mid - 1;
      } else {
        const double mx = c3[1] / c3[0], my = c3[2] / c3[0];
        double p3[3] = {0, 0, 0};
        for (int j = tid; j < N; j += blockDim.x) {
          const double f = fv[j], s = sv[j];
          if (f < t1 || s < t2) { const double dx = f - mx, dy = s - my; p3[0] += dx * dx; p3[1] += dy * dy; p3[2] += dx * dy; }
        }
        block_sum_vec_all<3>(p3, vec);
        // r = clip(p3[2] / (sqrt(p3[0]) sqrt(p3[1])), -1, 1) is only ever compared with 0: its sign is p3[2]'s, and it is NaN
        // (neither bound moves) exactly when one of the variances is 0 — two fp64 square roots and a division less per
        // probe, executed by every lane (the scalar fp64 arithmetic of a probe cost more than its passes over the pixels)
        if (p3[0] != 0 && p3[1] != 0) {
          if (p3[2] < 0) left = mid - 1;
          else if (p3[2] >= 0) { right = mid + 1; valid = mid; }
        }
      }
      lastmid = mid;
      mid = costes_next_mid(left, right, int_bounds);
    }
    const double t1 = (valid - 1) / scale_max, t2 = ca * t1 + cb;
    double c4[4] = {0, 0, 0, 0};
    int f_any = 0, s_any = 0, c_any = 0;
    for (int j = tid; j < N; j += blockDim.x) {
      const double f = fv[j], s = sv[j];
      const bool fa = f > t1, sa = s > t2;
      f_any |= fa; s_any |= sa;
      if (f >= t1) c4[0] += f;
      if (s >= t2) c4[1] += s;
      if (fa && sa) { c4[2] += f; c4[3] += s; c_any = 1; }
    }
    block_sum_vec_all<4>(c4, vec);
    const int FA = block_max_i32(f_any, red_i), SA = block_max_i32(s_any, red_i), CA = block_max_i32(c_any, red_i);
    if (tid == 0) {
      const double d1 = FA ? c4[0] : 0.0, d2 = SA ? c4[1] : 0.0;
      out[col_costes] = CA ? c4[2] / d1 : 0.0;
      out[col_costes + 1] = CA ? c4[3] / d2 : 0.0;
    }
  }
}

#endif  // __HIPCC__
