// bbm_amd/csrc/eval_world.hpp -- eval / pdf / eval + pdf in world space: `in` and `out` in world space and one shading
// normal per lane, the frame (frame.hpp) built and applied in registers ahead of the model (bbm_hip_eval_pdf_world and
// its material table twin bbm_hip_eval_pdf_table_world).  This is a path tracer's next-event
// estimation at a hit: eval(in, out), pdf(in, out) and the cosine of `in` against the normal.  Included at the end of
// kernels.hpp, after lanes.hpp.
//
// Lane i returns what bbm_hip_frame_to_local(normal, in), bbm_hip_frame_to_local(normal, out) and the local call
// return for it in sequence, bit for bit (frame_pair, kernels.hpp); cos[i] is the z of the first.  The local
// directions never leave the registers: 52 B per lane (56 with the cosine) instead of 112 in three launches.
//
// Layout of the uniform kernels: k_eval_pdf_v4's and k_eval_pdf_v1's, with three more 16-byte loads per quad and one
// more 16-byte store where the cosine is asked for.  The three modes are compile-time, as there; the mask and the
// cosine are runtime, wave-uniform arguments, so a row has one quad and one one-lane kernel per mode, times the exact
// variant where it has one.  The frame is needed only ahead of the model: the pair is transformed, the cosine stored,
// and the nine frame floats are dead before the evaluation starts.  The compact rows (compact_eval) run
// k_eval_pdf_compact<FRAME>, the table call the per-lane kernels of lanes.hpp over EvalTabWorldArgs.
//
// W = EvalTangentArgs: the tangent form (bbm_hip_eval_pdf_world_tangent) -- the frame of a normal and
// a tangent per lane (tangent_frame), three more 16-byte loads per quad.  Instantiated for the anisotropic rows only
// (models.hpp), none of which is a compact row.  With W = EvalWorldArgs the kernels hold nothing of it.
#pragma once

namespace bbmhip {

// Whether the quad form is used for aligned arrays, per mode (EXACT: the kernel the exact mode launches), judged from
// the compiler's resource report on top of nothing: the local k_eval_pdf_v4 is always a quad.  A row whose world quad
// spills -- to scratch, or to AGPRs at fewer waves -- where its one-lane world kernel does not runs one lane per
// thread.  Specialised in models.hpp (as is eval_tab_world_quad, lanes.hpp).
template<class Model, int MODE, bool EXACT> struct eval_world_quad { static constexpr bool value = true; };
// the tangent form's, judged on top of it
template<class Model, int MODE, bool EXACT> struct eval_tangent_quad : eval_world_quad<Model, MODE, EXACT> {};
template<class Model, int MODE, bool EXACT, class W> constexpr bool eval_world_use_quad()
{
  if constexpr (tangent_args<W>) return eval_tangent_quad<Model, MODE, EXACT>::value;
  else return eval_world_quad<Model, MODE, EXACT>::value;
}

// Four pairs per thread-iteration: nine 16-byte nontemporal loads (in, out, the normal), the stores of k_eval_pdf_v4
// and the cosine's.  Every array 16-byte aligned and the mask 4-byte aligned (checked on the host); the n % 4 tail
// runs scalar.  The first quad's loads go out before the table prologue and the model's construction where the local
// kernel's do (eval_prefetch).
template<class Model, int MODE, bool EXACT, class W>
__global__ __launch_bounds__(kBlock) BBM_HIP_KERNEL_ATTR __attribute__((amdgpu_waves_per_eu(eval_waves<Model>::value, 8)))
void k_eval_pdf_world_v4(W w)
{
  const EvalArgs& a = w.e;
  const uint64_t n4 = a.n >> 2;
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  float4 ix, iy, iz, ox, oy, oz, wx, wy, wz;
  float4 tx = {}, ty = {}, tz = {};
  uint32_t mk = 0x01010101u;
  const auto load = [&](uint64_t q) {
    ix = ld4<true>(a.ix, q); iy = ld4<true>(a.iy, q); iz = ld4<true>(a.iz, q);
    ox = ld4<true>(a.ox, q); oy = ld4<true>(a.oy, q); oz = ld4<true>(a.oz, q);
    wx = ld4<true>(w.nx, q); wy = ld4<true>(w.ny, q); wz = ld4<true>(w.nz, q);
    if constexpr (tangent_args<W>) { tx = ld4<true>(w.tx, q); ty = ld4<true>(w.ty, q); tz = ld4<true>(w.tz, q); }
    if (a.mask) mk = reinterpret_cast<const uint32_t*>(a.mask)[q];
  };
  constexpr bool pf = eval_prefetch<Model>::value;
  if (pf && t < n4) load(t);
  if constexpr (uses_math_tables<Model>::value) math_tables_init();
#ifdef BBM_HIP_TABLES_POISON
  else math_tables_poison();
#endif
  const Model m(a.p.v);
  for (bool first = true; t < n4; t += stride, first = false)
  {
    if (!pf || !first) load(t);
    const float nnx[4] = {wx.x, wx.y, wx.z, wx.w}, nny[4] = {wy.x, wy.y, wy.z, wy.w}, nnz[4] = {wz.x, wz.y, wz.z, wz.w};
    float inx[4] = {ix.x, ix.y, ix.z, ix.w}, iny[4] = {iy.x, iy.y, iy.z, iy.w}, inz[4] = {iz.x, iz.y, iz.z, iz.w};
    float onx[4] = {ox.x, ox.y, ox.z, ox.w}, ony[4] = {oy.x, oy.y, oy.z, oy.w}, onz[4] = {oz.x, oz.y, oz.z, oz.w};
    const float ttx[4] = {tx.x, tx.y, tx.z, tx.w}, tty[4] = {ty.x, ty.y, ty.z, ty.w}, ttz[4] = {tz.x, tz.y, tz.z, tz.w};
    bool in_frame[4];
    // every pair into its frame first: the frames are dead before the first evaluation
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      v3 in = mk3(inx[j], iny[j], inz[j]), out = mk3(onx[j], ony[j], onz[j]);
      if constexpr (tangent_args<W>)
        in_frame[j] = frame_pair(mk3(nnx[j], nny[j], nnz[j]), mk3(ttx[j], tty[j], ttz[j]), ((mk >> (8 * j)) & 0xffu) != 0, in, out);
      else in_frame[j] = frame_pair(mk3(nnx[j], nny[j], nnz[j]), ((mk >> (8 * j)) & 0xffu) != 0, in, out);
      inx[j] = in.x; iny[j] = in.y; inz[j] = in.z;
      onx[j] = out.x; ony[j] = out.y; onz[j] = out.z;
    }
    if (w.cos) st4<true>(w.cos, t, inz[0], inz[1], inz[2], inz[3]);
    float r[4], g[4], b[4], p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      float rgb[3];
      model_eval_pdf<MODE, EXACT>(m, mk3(inx[j], iny[j], inz[j]), mk3(onx[j], ony[j], onz[j]),
                                  in_frame[j] ? a.component : 0u, rgb, p[j]);
      r[j] = rgb[0]; g[j] = rgb[1]; b[j] = rgb[2];
    }
    if (MODE & kModeEval)
    {
      st4<true>(a.r, t, r[0], r[1], r[2], r[3]);
      st4<true>(a.g, t, g[0], g[1], g[2], g[3]);
      st4<true>(a.b, t, b[0], b[1], b[2], b[3]);
    }
    if (MODE & kModePdf) st4<true>(a.pdf, t, p[0], p[1], p[2], p[3]);
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x < (a.n & 3))
  {
    const uint64_t i = (n4 << 2) + threadIdx.x;
    one_pair_world<Model, MODE, EXACT>(m, w, i, a.mask ? (a.mask[i] != 0) : true, true);
  }
}

// One pair per thread: unaligned arrays, and the rows eval_world_quad excludes.
template<class Model, int MODE, bool EXACT, class W>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(eval_waves<Model>::value, 8)))
void k_eval_pdf_world_v1(W w)
{
  math_tables_init();
  const EvalArgs& a = w.e;
  const Model m(a.p.v);
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < a.n; i += stride)
    one_pair_world<Model, MODE, EXACT>(m, w, i, a.mask ? (a.mask[i] != 0) : true, true);
}

template<class Model, int MODE, bool EXACT, class W>
void launch_world_kernel(const W& w, bool aligned, hipStream_t s)
{
  constexpr bool quad = eval_world_use_quad<Model, MODE, EXACT, W>();
  const bool vec = quad && aligned;
  const uint64_t units = vec ? (w.e.n >> 2) : w.e.n;
  uint64_t blocks = (units + kBlock - 1) / kBlock;
  if (blocks < 1) blocks = 1;
  if (blocks > max_blocks()) blocks = max_blocks();
  if (eval_grid_cap<Model>::value && blocks > eval_grid_cap<Model>::value) blocks = eval_grid_cap<Model>::value;
  if constexpr (quad)
  {
    if (vec) hipLaunchKernelGGL((k_eval_pdf_world_v4<Model, MODE, EXACT, W>), dim3(unsigned(blocks)), dim3(kBlock), 0, s, w);
  }
  if (!vec) hipLaunchKernelGGL((k_eval_pdf_world_v1<Model, MODE, EXACT, W>), dim3(unsigned(blocks)), dim3(kBlock), 0, s, w);
}

// launch_mode's host work and ladder: compaction for the rows that have it, else the exact or the default kernel
template<class Model, int MODE, class W>
int launch_mode_world(const W& w0, hipStream_t s)
{
  if (const int rc = host_prepare<Model>::run(s)) return rc;
  if (const int rc = host_validate<Model>::run(w0.e.p)) return rc;
  W w = w0;
  EvalArgs& a = w.e;
  void* scratch = nullptr;
  if (MODE & kModePdf)
    if (const int rc = host_params<Model>::run(a.p, a.component, s, &scratch)) return rc;
  struct Release { void* p; hipStream_t s; ~Release() { host_params<Model>::done(p, s); } } release{scratch, s};
  bool vec = aligned16(a.ix) && aligned16(a.iy) && aligned16(a.iz) && aligned16(a.ox) && aligned16(a.oy) &&
             aligned16(a.oz) && aligned16(w.nx) && aligned16(w.ny) && aligned16(w.nz) && aligned16(w.cos) &&
             (reinterpret_cast<uintptr_t>(a.mask) & 3u) == 0;
  if (MODE & kModeEval) vec = vec && aligned16(a.r) && aligned16(a.g) && aligned16(a.b);
  if (MODE & kModePdf) vec = vec && aligned16(a.pdf);
  if constexpr (tangent_args<W>) vec = vec && aligned16(w.tx) && aligned16(w.ty) && aligned16(w.tz);
  static_assert(!(tangent_args<W> && compact_eval<Model>::value), "no compact row is anisotropic");
  bool compact = false;
  if constexpr (compact_eval<Model>::value) compact = vec && use_compact();
  if (compact)
  {
    uint64_t blocks = ((a.n >> 2) + kBlock - 1) / kBlock;
    if (blocks < 1) blocks = 1;
    if (blocks > max_blocks()) blocks = max_blocks();
    if (eval_grid_cap<Model>::value && blocks > eval_grid_cap<Model>::value) blocks = eval_grid_cap<Model>::value;
    if constexpr (compact_eval<Model>::value)       // instantiated for the rows that have it only
      hipLaunchKernelGGL((k_eval_pdf_compact<Model, MODE, true, true>), dim3(unsigned(blocks)), dim3(kBlock), 0, s, w);
  }
  else if (exact_launch<Model>())
  {
    if constexpr (model_has_exact<Model>()) launch_world_kernel<Model, MODE, true, W>(w, vec, s);
  }
  else launch_world_kernel<Model, MODE, false, W>(w, vec, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("kernel launch failed: ") + hipGetErrorString(e));
  return BBM_HIP_OK;
}

template<class Model, class W>
int launch_eval_pdf_world_args(const W& w, int mode, hipStream_t s)
{
  switch (mode)
  {
    case kModeEval: return launch_mode_world<Model, kModeEval, W>(w, s);
    case kModePdf: return launch_mode_world<Model, kModePdf, W>(w, s);
    default: return launch_mode_world<Model, kModeEvalPdf, W>(w, s);
  }
}

template<class Model>
int launch_eval_pdf_world(const EvalWorldArgs& w, int mode, hipStream_t s) { return launch_eval_pdf_world_args<Model>(w, mode, s); }
// the tangent form; instantiated for the anisotropic rows only
template<class Model>
int launch_eval_pdf_tangent(const EvalTangentArgs& w, int mode, hipStream_t s) { return launch_eval_pdf_world_args<Model>(w, mode, s); }

// the table call: the per-lane kernels over EvalTabWorldArgs (lanes.hpp)
template<class Model>
int launch_eval_pdf_tab_world(const EvalTabWorldArgs& a, int mode, hipStream_t s)
{
  return launch_eval_pdf_lanes<Model, EvalTabWorldArgs>(a, mode, s);
}
template<class Model>
int launch_eval_pdf_tab_tangent(const EvalTabTangentArgs& a, int mode, hipStream_t s)
{
  return launch_eval_pdf_lanes<Model, EvalTabTangentArgs>(a, mode, s);
}

}  // namespace bbmhip
