// object_launch.h — the launch front end of the 2-D feature kernels that work on one object per workgroup (feat_intensity.hip,
// feat_texture.hip, feat_coloc.hip, feat_cell.hip, feat_shape.hip, feat_zernike.hip, feat_radial.hip, feat_localisation.hip).
// Host side only; the counterparts on volume labels are volume_launch in volume_table.h (one object per workgroup) and
// volume_pass.h (the kernels that walk a whole stack).
//
// Every such kernel exists in two forms, <GLOBAL = false> and <GLOBAL = true>, with one argument struct that carries
// `unsigned char* gscratch`:
//   LDS form     one workgroup per object, aliby_pick_block(work) threads, the working set (`need` bytes, sized from the object
//                table's max_h / max_w / max_area) in dynamic LDS; gscratch = nullptr.  Taken when need <= the site's LDS budget.
//                The budgets stay with the sites: they follow from each kernel's static LDS and occupancy.
//   global form  at most OBJECT_GLOBAL_BLOCKS workgroups of 256 threads striding over the objects, workgroup b's working set at
//                gscratch + b * need inside ctx->scratch; no dynamic LDS.
//
// The scratch rule.  A global-form launch borrows ctx->scratch until the stream has passed it, and the next one (or any other
// user of the context's scratch) may move or overwrite the block: only ONE may be in flight per context.  Launches on one
// stream are ordered, and a thread has a context of its own (aliby_amd/_lib.py, default_context); what must not happen is two
// streams of one context running global forms side by side.  Whoever sends per-object launches of one context to several streams
// (_FanOut in aliby_amd/extraction/families.py, the early colocalisation launch of aliby_amd/runner.py) asks
// ObjectTable.lds_resident (aliby_amd/extraction/engine.py) first: max_h * max_w <= 4096, which keeps every box-sized and area-sized
// site in LDS.  It does not by itself keep k_shape_hull there: its working set grows with max_h alone (about 152 max_h bytes), so
// a box taller than about 646 rows and at most 6 wide passes that test and still sends the hull to the global form.  That is
// harmless today only because one hull launch (sizeshape or feret) is in flight per evaluation.
//
// hipFuncAttributeMaxDynamicSharedMemorySize is raised when need exceeds OBJECT_LDS_ATTR_ABOVE = 32 KiB.  The sites used to
// spell 32 or 48 KiB; 32 KiB, the lower, costs the former 48 KiB sites one more hipFuncSetAttribute per launch for working
// sets between the two — nothing the benchmark's objects (a few KiB) reach — and cannot change a result.
#pragma once
#include "common.h"

#ifdef __HIPCC__
#define OBJECT_GLOBAL_BLOCKS 512
#define OBJECT_LDS_ATTR_ABOVE (32 * 1024)

namespace {

// the kernel of the planes' pixel type (ALIBY_U16 / ALIBY_F32), for kernels templated on it
template <class Args>
inline void (*object_kernel(int dtype, void (*k_u16)(Args), void (*k_f32)(Args)))(Args) {
  return dtype == ALIBY_U16 ? k_u16 : k_f32;
}

// One launch of a per-object kernel in the form that `need` bytes against `lds_budget` selects; sets a.gscratch.  `work` = the
// pixels a workgroup of the LDS form loops over (what aliby_pick_block sizes the workgroup by).
template <class Args>
int object_launch(aliby_ctx* ctx, void (*k_lds)(Args), void (*k_global)(Args), Args& a, int n_obj, size_t need, size_t lds_budget,
                  long long work, hipStream_t s) {
  if (need <= lds_budget) {
    a.gscratch = nullptr;
    if (need > OBJECT_LDS_ATTR_ABOVE) HIP_TRY(hipFuncSetAttribute((const void*)k_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
    hipLaunchKernelGGL(k_lds, dim3(n_obj), dim3(aliby_pick_block(work)), need, s, a);
  } else {
    const int g = n_obj < OBJECT_GLOBAL_BLOCKS ? n_obj : OBJECT_GLOBAL_BLOCKS;
    const int rc = aliby_ensure_scratch(ctx, (size_t)g * need);
    if (rc) return rc;
    a.gscratch = (unsigned char*)ctx->scratch;
    hipLaunchKernelGGL(k_global, dim3(g), dim3(256), 0, s, a);
  }
  KERNEL_CHECK();
  return ALIBY_OK;
}

}  // namespace
#endif  // __HIPCC__
