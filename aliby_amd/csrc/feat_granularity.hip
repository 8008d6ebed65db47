// feat_granularity.hip — cp_measure "granularity" (CellProfiler MeasureGranularity; bound at
// src/extraction/core/functions/loaders.py:71-73 like every core measurement, outside the builder's default list).
//
// The reference evaluates it once per object on a full-frame single-object label image (extract.py:147-153).  Everything up to the
// per-object means is a property of the IMAGE (with CellProfiler's default, whole-frame image mask): granularity_pass.h describes it
// and runs it once per (tile, channel), as the DIM = 2 instantiation of what this file shares with feat_granularity3d.hip.  Here are
// the image mask "objects" (its two kernels), the per-object means over aliby_object rows, and the entry.
//
// Restated in oracle/granularity_restated.py; its primitives are pinned against scikit-image 0.18.3, the measurement as a whole is
// PARITY UNPINNED (cp_measure is not available offline).
#include "granularity_pass.h"

typedef unsigned short u16;

namespace {

// mask of the subsampled frame when the image mask is "objects": bilinear sample of (labels > 0) > 0.9 (mask_order = 1), at i / size
// like k_gran_sample
__global__ void k_gran_sample_mask(const u16* __restrict__ labels, GranGeom g, double size, unsigned char* __restrict__ dst) {
  const size_t total = gran_count<2>(g.F, g.sub), plane = (size_t)g.src.h * g.src.w;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const GranIndex v = gran_index<2>(i, g.sub);
    const u16* p = labels + (size_t)v.f * plane;
    dst[i] = lerp<2>([&](int, int yy, int xx) { return p[(size_t)yy * g.src.w + xx] ? 1.0 : 0.0; }, g.src, 0.0, (double)v.y / size,
                     (double)v.x / size) > 0.9;
  }
}
// ... and of the background grid: the same rule on that mask
__global__ void k_gran_resample_mask(const unsigned char* __restrict__ src, int F, GranExtent from, GranExtent to, double size,
                                     unsigned char* __restrict__ dst) {
  const size_t total = gran_count<2>(F, to);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const GranIndex v = gran_index<2>(i, to);
    const unsigned char* p = src + (size_t)v.f * from.h * from.w;
    dst[i] = lerp<2>([&](int, int yy, int xx) { return (double)p[(size_t)yy * from.w + xx]; }, from, 0.0, (double)v.y / size,
                     (double)v.x / size) > 0.9;
  }
}

struct GranMeanArgs {
  const u16* labels;
  const aliby_object* tab;
  int n_obj;
  GranGeom g;
  const void* planes;  // STEP0: the original pixels (typed)
  int C, channel;
  const double* rec;   // STEP > 0: [F, sh, sw]
  double sy, sx;       // frame -> subsampled coordinates ((sh - 1) / (Y - 1), ...)
  double* prev;        // [n_obj] mean of the previous step (updated)
  double* start;       // [n_obj] max(mean_0, eps) (written by step 0)
  double* out;         // feature matrix
  int ld, col;         // column of this step
};

// one wave per object: mean over the object's pixels of the (resized) image, lanes stride the bbox, fixed reduction order
template <typename T, bool STEP0>
__global__ __launch_bounds__(64) void k_gran_means(GranMeanArgs a) {
  const int lane = threadIdx.x;
  const int X = a.g.src.w;
  const size_t plane = (size_t)a.g.src.h * X;
  for (int oi = blockIdx.x; oi < a.n_obj; oi += gridDim.x) {
    const aliby_object o = a.tab[oi];
    double s = 0.0;
    if (o.area > 0) {
      const u16* lab = a.labels + (size_t)o.tile * plane;
      const int h = o.y1 - o.y0, w = o.x1 - o.x0;
      const u16 L = (u16)o.label;
      const T* px = STEP0 ? reinterpret_cast<const T*>(a.planes) + ((size_t)o.tile * a.C + a.channel) * plane : nullptr;
      const double* rec = STEP0 ? nullptr : a.rec + (size_t)o.tile * a.g.sub.h * a.g.sub.w;
      for (int i = lane; i < h * w; i += 64) {
        const int yy = o.y0 + i / w, xx = o.x0 + i % w;
        const size_t idx = (size_t)yy * X + xx;
        if (lab[idx] != L) continue;
        if (STEP0) s += (double)px_load<T>(px, idx);
        else s += lerp<2>([&](int, int y2, int x2) { return rec[(size_t)y2 * a.g.sub.w + x2]; }, a.g.sub, 0.0, (double)yy * a.sy, (double)xx * a.sx);
      }
    }
    s = wave_sum(s);
    if (lane == 0) gran_means_write<STEP0>(s, o.area, a.prev + oi, a.start + oi, a.out + (size_t)oi * a.ld + a.col);
  }
}

// the images, then the masks of the two grids
size_t gran_bytes(const GranGeom& g, int n_obj) { return gran_image_bytes(g, n_obj) + gran_count(g.F, g.sub) + gran_count(g.F, g.back) + 64; }

}  // namespace

extern "C" size_t aliby_granularity_workspace_bytes(int F, int Y, int X, int n_obj, double subsample_size, double image_sample_size) {
  if (F <= 0 || Y <= 0 || X <= 0 || n_obj < 0 || !(subsample_size > 0) || !(image_sample_size > 0)) return 0;
  return gran_bytes(gran_geometry(F, GranExtent{1, Y, X}, subsample_size, image_sample_size), n_obj);
}

extern "C" int aliby_features_granularity(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C, int Y,
                                          int X, int channel, const aliby_object* table_dev, int n_obj, double subsample_size,
                                          double image_sample_size, int element_size, int spectrum_length, int image_mask_objects,
                                          void* workspace, size_t workspace_bytes, double* out, int ld, int col0, void* stream_) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  if (n_obj == 0) return ALIBY_OK;
  ARG_CHECK(labels && planes && table_dev && out, "NULL argument");
  ARG_CHECK(F > 0 && Y > 1 && X > 1, "bad shape");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "dtype must be ALIBY_U16 or ALIBY_F32");
  ARG_CHECK(channel >= 0 && channel < C, "channel out of range");
  ARG_CHECK(subsample_size > 0 && subsample_size <= 1 && image_sample_size > 0 && image_sample_size <= 1, "sample sizes must be in (0, 1]");
  ARG_CHECK(element_size >= 1 && element_size <= 64 && spectrum_length >= 1 && spectrum_length <= 64, "element_size / spectrum length out of range");
  ARG_CHECK(col0 >= 0 && col0 + spectrum_length <= ld, "columns exceed row stride");
  hipStream_t s = as_stream(stream_);
  const GranGeom g = gran_geometry(F, GranExtent{1, Y, X}, subsample_size, image_sample_size);
  ARG_CHECK(g.sub.h > 1 && g.sub.w > 1 && g.back.h > 1 && g.back.w > 1, "frame too small for these sample sizes");
  ARG_CHECK(workspace != nullptr && workspace_bytes >= gran_bytes(g, n_obj), "workspace smaller than aliby_granularity_workspace_bytes()");
  ARG_CHECK(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  const GranBuffers b = gran_carve(workspace, g, n_obj);
  // the image mask "objects" on the subsampled frame and, where the background is resized, on its grid
  unsigned char *msk = nullptr, *bmsk = nullptr;
  if (image_mask_objects) {
    const size_t ns = gran_count(F, g.sub), nb = gran_count(F, g.back);
    bmsk = msk = b.tail;
    hipLaunchKernelGGL(k_gran_sample_mask, dim3(gran_grid(ns)), dim3(256), 0, s, labels, g, subsample_size, msk);
    if (image_sample_size < 1) {
      bmsk = msk + ns;
      hipLaunchKernelGGL(k_gran_resample_mask, dim3(gran_grid(nb)), dim3(256), 0, s, msk, F, g.sub, g.back, image_sample_size, bmsk);
    }
  }
  GranMeanArgs m;
  m.labels = labels; m.tab = table_dev; m.n_obj = n_obj; m.g = g; m.planes = planes; m.C = C; m.channel = channel; m.rec = nullptr;
  m.sy = gran_scale(g.sub.h, Y); m.sx = gran_scale(g.sub.w, X);
  m.prev = b.prev; m.start = b.start; m.out = out; m.ld = ld; m.col = col0;
  const unsigned og = (unsigned)(n_obj < 65535 ? n_obj : 65535);
  auto means = [&](int step, const double* rec) {
    m.rec = rec;
    m.col = col0 + (step ? step - 1 : 0);
    if (step) hipLaunchKernelGGL((k_gran_means<u16, false>), dim3(og), dim3(64), 0, s, m);  // (T is unused when STEP0 is false)
    else if (dtype == ALIBY_U16) hipLaunchKernelGGL((k_gran_means<u16, true>), dim3(og), dim3(64), 0, s, m);
    else hipLaunchKernelGGL((k_gran_means<float, true>), dim3(og), dim3(64), 0, s, m);
  };
  return gran_run<2>(g, planes, dtype, C, channel, subsample_size, image_sample_size, element_size, spectrum_length, b, msk, bmsk, nullptr,
                     "granularity", means, s);
}
