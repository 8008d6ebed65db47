// feat_granularity3d.hip — "granularity3d": the granular spectrum of feat_granularity.hip (CellProfiler MeasureGranularity) on
// labelled stacks [F, Z, Y, X], CellProfiler's volumetric branch recalled (PARITY UNPINNED; restated in tests/granularity3d_ref.py,
// defined in include/aliby_hip.h).  The image pipeline and the spectrum are the DIM = 3 instantiation of granularity_pass.h, which
// describes them; every stack is on its own.  The image mask is the whole stack (CellProfiler's default); the "objects" mask of the
// 2-D family is not built.
//
// Here are the per-object means and the entry.  The means take their bounding boxes from the shared volume table (volume_table.h),
// built in the caller's workspace: one wave per (stack, label) row, the lanes stride the box in raster order, fixed reduction order —
// a row carries the same bits whatever the run, the other stacks of the call and the batch.  The entry waits on its stream (the change
// flag of the reconstruction): a main-stream call.
#include "granularity_pass.h"
#include "volume_table.h"

typedef unsigned short u16;

#define GRANULARITY3D_MAX_ELEMENT 16  // bounds the per-voxel scan of the ball (about 17 k offsets at 16); not a structural limit
#define GRANULARITY3D_MAX_LENGTH 64

namespace {

struct Gran3MeanArgs {
  VolumeArgs v;        // labels, shape, offsets and the table (n_items = rows)
  GranGeom g;
  const void* pixels;  // STEP0: the original pixels (typed)
  int C, channel;
  const double* rec;   // STEP > 0: [F, sz, sh, sw]
  double cz, cy, cx;   // stack -> subsampled coordinates ((sz - 1) / (Z - 1), ...; 0 on an axis of length 1)
  double* prev;        // [rows] mean of the previous step (updated)
  double* start;       // [rows] max(mean_0, eps) (written by step 0)
  double* out;         // feature matrix
  int ld, col;         // column of this step
};

// one wave per row: mean over the object's voxels of the (resized) image; the lanes stride the bounding box in raster order, fixed
// reduction order.  A row without voxels gets NaN.
template <typename T, bool STEP0>
__global__ __launch_bounds__(64) void k_g3_means(Gran3MeanArgs a) {
  const int lane = threadIdx.x;
  const int Y = a.v.Y, X = a.v.X;
  const size_t vol = (size_t)a.v.Z * Y * X;
  for (int row = blockIdx.x; row < a.v.n_items; row += gridDim.x) {
    const unsigned count = a.v.count[row];
    double s = 0.0;
    if (count > 0) {
      const int f = volume_stack_of(a.v.offsets, a.v.F, row);
      const u16 L = (u16)(row - a.v.offsets[f] + 1);
      const u16* lab = a.v.labels + (size_t)f * vol;
      const VolumeBox box = volume_box(a.v.bmin, a.v.bmax, row);
      const T* px = STEP0 ? reinterpret_cast<const T*>(a.pixels) + ((size_t)f * a.C + a.channel) * vol : nullptr;
      const double* rec = STEP0 ? nullptr : a.rec + (size_t)f * a.g.sub.d * a.g.sub.h * a.g.sub.w;
      for (unsigned i = lane; i < box.nbox; i += 64) {
        const unsigned r = i / box.w;
        const int xx = (int)(box.x0 + i % box.w), yy = (int)(box.y0 + r % box.h), zz = (int)(box.z0 + r / box.h);
        const size_t idx = ((size_t)zz * Y + yy) * X + xx;
        if (lab[idx] != L) continue;
        if (STEP0) s += (double)px_load<T>(px, idx);
        else s += lerp<3>([&](int z2, int y2, int x2) { return rec[((size_t)z2 * a.g.sub.h + y2) * a.g.sub.w + x2]; }, a.g.sub, (double)zz * a.cz,
                          (double)yy * a.cy, (double)xx * a.cx);
      }
    }
    s = wave_sum(s);
    if (lane == 0) gran_means_write<STEP0>(s, count, a.prev + row, a.start + row, a.out + (size_t)row * a.ld + a.col);
  }
}

// the images, then the object table (7 words a row) and the offsets
size_t g3_bytes(const GranGeom& g, int rows) { return gran_image_bytes(g, rows) + ((size_t)rows * 7 + (size_t)g.F + 1) * 4; }

bool g3_sizes_ok(double subsample_size, double image_sample_size) {
  return subsample_size > 0 && subsample_size <= 1 && image_sample_size > 0 && image_sample_size <= 1;
}

}  // namespace

extern "C" size_t aliby_granularity3d_workspace_bytes(int F, int Z, int Y, int X, int rows, double subsample_size, double image_sample_size) {
  if (F <= 0 || Z <= 0 || Y <= 0 || X <= 0 || rows < 0 || !g3_sizes_ok(subsample_size, image_sample_size)) return 0;
  return g3_bytes(gran_geometry(F, GranExtent{Z, Y, X}, subsample_size, image_sample_size), rows);
}

extern "C" int aliby_features_granularity3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y,
                                            int X, int channel, const int32_t* offsets_host, double subsample_size, double image_sample_size,
                                            int element_size, int spectrum_length, void* workspace, size_t workspace_bytes,
                                            int32_t* sweeps_host, double* out, int ld, int col0, void* stream_) {
  ARG_CHECK(ctx && labels && pixels && offsets_host && out, "granularity3d: null argument");
  if (!volume_shape_ok("granularity3d", F, Z, Y, X, offsets_host, 1ull << 30)) return ALIBY_ERR_INVALID;
  ARG_CHECK(Y > 1 && X > 1, "granularity3d: Y and X must be above 1");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "granularity3d: dtype must be ALIBY_U16 or ALIBY_F32");
  ARG_CHECK(channel >= 0 && channel < C, "granularity3d: channel out of range");
  ARG_CHECK(g3_sizes_ok(subsample_size, image_sample_size), "granularity3d: sample sizes must be in (0, 1]");
  ARG_CHECK(element_size >= 1 && element_size <= GRANULARITY3D_MAX_ELEMENT, "granularity3d: element_size must lie in 1..16");
  ARG_CHECK(spectrum_length >= 1 && spectrum_length <= GRANULARITY3D_MAX_LENGTH, "granularity3d: spectrum length must lie in 1..64");
  ARG_CHECK(col0 >= 0 && (long long)col0 + spectrum_length <= ld, "granularity3d: columns exceed row stride");
  const GranGeom g = gran_geometry(F, GranExtent{Z, Y, X}, subsample_size, image_sample_size);
  ARG_CHECK(g.sub.h > 1 && g.sub.w > 1 && g.back.h > 1 && g.back.w > 1, "granularity3d: stack too small for these sample sizes");
  const int rows = offsets_host[F];
  if (sweeps_host) for (int k = 0; k < spectrum_length; ++k) sweeps_host[k] = 0;
  if (rows <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream_);
  ARG_CHECK(workspace != nullptr && workspace_bytes >= g3_bytes(g, rows), "workspace smaller than aliby_granularity3d_workspace_bytes()");
  ARG_CHECK(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  const GranBuffers b = gran_carve(workspace, g, rows);
  unsigned* table = (unsigned*)b.tail;
  int* offsets_dev = (int*)(table + (size_t)rows * 7);
  // the object table: voxel count and bounding box of every row
  HIP_TRY(hipMemcpyAsync(offsets_dev, offsets_host, sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s));
  const int rc = volume_table_launch(labels, F, Z, Y, X, offsets_dev, rows, table, s);
  if (rc) return rc;
  Gran3MeanArgs m;
  m.v = VolumeArgs{labels, F, Z, Y, X, offsets_dev, table, table + rows, table + (size_t)rows * 4, nullptr, rows};
  m.g = g; m.pixels = pixels; m.C = C; m.channel = channel; m.rec = nullptr;
  m.cz = gran_scale(g.sub.d, Z); m.cy = gran_scale(g.sub.h, Y); m.cx = gran_scale(g.sub.w, X);
  m.prev = b.prev; m.start = b.start; m.out = out; m.ld = ld; m.col = col0;
  const unsigned og = (unsigned)(rows < 65535 ? rows : 65535);
  auto means = [&](int step, const double* rec) {
    m.rec = rec;
    m.col = col0 + (step ? step - 1 : 0);
    if (step) hipLaunchKernelGGL((k_g3_means<u16, false>), dim3(og), dim3(64), 0, s, m);  // (T is unused when STEP0 is false)
    else if (dtype == ALIBY_U16) hipLaunchKernelGGL((k_g3_means<u16, true>), dim3(og), dim3(64), 0, s, m);
    else hipLaunchKernelGGL((k_g3_means<float, true>), dim3(og), dim3(64), 0, s, m);
  };
  return gran_run<3>(g, pixels, dtype, C, channel, subsample_size, image_sample_size, element_size, spectrum_length, b, nullptr, nullptr,
                     sweeps_host, "granularity3d", means, s);
}
