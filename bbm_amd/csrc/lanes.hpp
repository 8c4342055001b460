// bbm_amd/csrc/lanes.hpp -- the per-lane kernels: every lane evaluates the model at a parameter block of its own.
// One kernel family over a lane-parameter source `Src`, a compile-time policy with two implementations: VarRows
// (varying.hpp: one optional float row per parameter) and TabRef (table.hpp: an index into a
// table of prepared blocks, §4.15).  Included at the end of kernels.hpp, after both.
//
// What a source provides, all of it inlined (nothing goes through a pointer or a runtime switch between sources):
//   Lane, load_lane(i)            lane i's own state: nothing for the rows, the index for a table;
//   lane_block<S>(u, l, i, q)     its block q from the kernarg block u;
//   lane_live(l)                  whether it is live (rows: always; table: an index in range), ANDed with its mask;
//   Quad<S>, load_quad<S>(t), quad_block<S>(u, c, j, q), quad_live(c, j)   the same for the four lanes of a quad, the
//                                 state loaded with the direction loads (TabRef: the four indices as one load);
//   aligned(S), kHostPrepare, slots<Model>, quad<Model>   the host's side (launch_lane_kernel, launch_prepared).
// S is the slot count of the row's own model (Src::slots); the sample kernels take it as a template argument because
// their Model may be the row's exact-mode sampler twin.  A lane that is not live runs with the component cleared,
// which is what a lane with mask[i] == 0 is to the uniform kernels.
//
// Layout of the quad eval kernel: k_eval_pdf_v4's -- four consecutive pairs per thread, one 16-byte nontemporal load
// per direction array, the source's quad, 16-byte nontemporal stores, a scalar tail -- with the model built inside the
// j loop, so one model is live at a time.  Unaligned arrays, and the rows Src::quad excludes, take one pair per thread
// (k_eval_lane1).  sample and reflectance run one lane per thread, as k_reflectance does.  All grids are full: one
// trip per thread, no grid-stride loop.
//
// The rows' quad eval kernel (k_eval_pdf_var) is the one body that is not shared.  Its loops over the kernarg block
// and the row pointers stand in the kernel itself: the compiler then leaves the kernarg in the constant segment and
// loads a field where it is used.  Behind inlined members of the source the same loops are unrolled before they
// reach the kernel, the kernarg copy is split into scalars loaded at entry, and 15 instantiations change their
// occupancy or scratch (pdf-only CookTorrance 8 -> 5 waves); the table's kernels always had the split form (their
// gather was a function), so one body cannot reproduce both.
#pragma once
#include <type_traits>

namespace bbmhip {

template<class Args, class S> struct LaneArgs { using Src = S; using Call = Args; Args e; S src; };

// named, so that a kernel's symbol carries a short name and not the template's
struct EvalVarArgs : LaneArgs<EvalArgs, VarRows> {};
struct SampleVarArgs : LaneArgs<SampleArgs, VarRows> {};
struct ReflVarArgs : LaneArgs<ReflArgs, VarRows> {};
struct EvalTabArgs : LaneArgs<EvalArgs, TabRef> {};      // e.p: the fallback block (and the aggregate mode slot)
struct SampleTabArgs : LaneArgs<SampleArgs, TabRef> {};
struct ReflTabArgs : LaneArgs<ReflArgs, TabRef> {};
// The world-space table call (bbm_hip_eval_pdf_table_world): the eval kernels below over
// EvalWorldArgs.  The frame is a property of the argument type (lane_frame), so the local instantiations keep their
// names and hold nothing of it.  Instantiated for TabRef only: there is no world-space call over rows.
struct EvalTabWorldArgs : LaneArgs<EvalWorldArgs, TabRef> {};
// Its tangent form (bbm_hip_eval_pdf_table_world_tangent): the frame of a normal and a tangent per
// lane (lane_tangent), for the anisotropic rows only.
struct EvalTabTangentArgs : LaneArgs<EvalTangentArgs, TabRef> {};
template<class A> constexpr bool lane_tangent = std::is_same_v<typename A::Call, EvalTangentArgs>;
template<class A> constexpr bool lane_frame = std::is_same_v<typename A::Call, EvalWorldArgs> || lane_tangent<A>;

template<class Model, int MODE, bool EXACT, class A>
__device__ __forceinline__ void lane_one_pair(const A& a, uint64_t i)
{
  constexpr int S = A::Src::template slots<Model>;
  const EvalArgs& e = eval_args_of(a.e);
  const auto l = a.src.load_lane(i);
  ParamBlock q;
  a.src.template lane_block<S>(e.p, l, i, q);
  const Model m(q.v);
  if constexpr (lane_frame<A>) one_pair_world<Model, MODE, EXACT>(m, a.e, i, e.mask ? (e.mask[i] != 0) : true, a.src.lane_live(l));
  else
  {
    float rgb[3], pdf;
    bool active = e.mask ? (e.mask[i] != 0) : true;
    active = active && a.src.lane_live(l);
    model_eval_pdf<MODE, EXACT>(m, mk3(e.ix[i], e.iy[i], e.iz[i]), mk3(e.ox[i], e.oy[i], e.oz[i]),
                                active ? e.component : 0u, rgb, pdf);
    if (MODE & kModeEval) { e.r[i] = rgb[0]; e.g[i] = rgb[1]; e.b[i] = rgb[2]; }
    if (MODE & kModePdf) e.pdf[i] = pdf;
  }
}

// Four pairs per thread; every float array and the source's own 16-byte aligned, the mask 4-byte aligned.
// lane_frame<A>: three more loads (the normal), the pair taken into its frame before the model is built, and one
// more store where the cosine is asked for (runtime, wave-uniform).
template<class Model, int MODE, bool EXACT, class A>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(eval_waves<Model>::value, 8)))
void k_eval_lane4(A a)
{
  math_tables_init();
  constexpr int S = A::Src::template slots<Model>;
  const EvalArgs& e = eval_args_of(a.e);
  const uint64_t n4 = e.n >> 2;
  const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t < n4)
  {
    const float4 ix = ld4<true>(e.ix, t), iy = ld4<true>(e.iy, t), iz = ld4<true>(e.iz, t);
    const float4 ox = ld4<true>(e.ox, t), oy = ld4<true>(e.oy, t), oz = ld4<true>(e.oz, t);
    float4 wx = {}, wy = {}, wz = {};
    if constexpr (lane_frame<A>) { wx = ld4<true>(a.e.nx, t); wy = ld4<true>(a.e.ny, t); wz = ld4<true>(a.e.nz, t); }
    float4 tx = {}, ty = {}, tz = {};
    if constexpr (lane_tangent<A>) { tx = ld4<true>(a.e.tx, t); ty = ld4<true>(a.e.ty, t); tz = ld4<true>(a.e.tz, t); }
    const auto c = a.src.template load_quad<S>(t);
    const uint32_t mk = e.mask ? reinterpret_cast<const uint32_t*>(e.mask)[t] : 0x01010101u;
    float inx[4] = {ix.x, ix.y, ix.z, ix.w}, iny[4] = {iy.x, iy.y, iy.z, iy.w}, inz[4] = {iz.x, iz.y, iz.z, iz.w};
    float onx[4] = {ox.x, ox.y, ox.z, ox.w}, ony[4] = {oy.x, oy.y, oy.z, oy.w}, onz[4] = {oz.x, oz.y, oz.z, oz.w};
    bool in_frame[4] = {true, true, true, true};
    if constexpr (lane_frame<A>)
    {
      // every pair into its frame first (frame_pair): the frames are dead before the first model is built
      const float nnx[4] = {wx.x, wx.y, wx.z, wx.w}, nny[4] = {wy.x, wy.y, wy.z, wy.w}, nnz[4] = {wz.x, wz.y, wz.z, wz.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
      {
        v3 in = mk3(inx[j], iny[j], inz[j]), out = mk3(onx[j], ony[j], onz[j]);
        if constexpr (lane_tangent<A>)
        {
          const float ttx[4] = {tx.x, tx.y, tx.z, tx.w}, tty[4] = {ty.x, ty.y, ty.z, ty.w}, ttz[4] = {tz.x, tz.y, tz.z, tz.w};
          in_frame[j] = frame_pair(mk3(nnx[j], nny[j], nnz[j]), mk3(ttx[j], tty[j], ttz[j]), ((mk >> (8 * j)) & 0xffu) != 0, in, out);
        }
        else in_frame[j] = frame_pair(mk3(nnx[j], nny[j], nnz[j]), ((mk >> (8 * j)) & 0xffu) != 0, in, out);
        inx[j] = in.x; iny[j] = in.y; inz[j] = in.z;
        onx[j] = out.x; ony[j] = out.y; onz[j] = out.z;
      }
      if (a.e.cos) st4<true>(a.e.cos, t, inz[0], inz[1], inz[2], inz[3]);
    }
    float r[4], g[4], b[4], p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      ParamBlock q;
      a.src.template quad_block<S>(e.p, c, j, q);
      const Model m(q.v);
      float rgb[3];
      bool active = (mk >> (8 * j)) & 0xffu;
      if constexpr (lane_frame<A>) active = in_frame[j];
      active = active && a.src.quad_live(c, j);
      const uint32_t comp = active ? e.component : 0u;
      model_eval_pdf<MODE, EXACT>(m, mk3(inx[j], iny[j], inz[j]), mk3(onx[j], ony[j], onz[j]), comp, rgb, p[j]);
      r[j] = rgb[0]; g[j] = rgb[1]; b[j] = rgb[2];
    }
    if (MODE & kModeEval)
    {
      st4<true>(e.r, t, r[0], r[1], r[2], r[3]);
      st4<true>(e.g, t, g[0], g[1], g[2], g[3]);
      st4<true>(e.b, t, b[0], b[1], b[2], b[3]);
    }
    if (MODE & kModePdf) st4<true>(e.pdf, t, p[0], p[1], p[2], p[3]);
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x < (e.n & 3)) lane_one_pair<Model, MODE, EXACT>(a, (n4 << 2) + threadIdx.x);
}

// The rows' quad: the same layout with the rows' loops in the kernel's own body (see the head of this file); one
// 16-byte nontemporal load per varying row, `vp[k] != nullptr` wave-uniform, every lane live.
template<class Model, int MODE, bool EXACT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(eval_waves<Model>::value, 8)))
void k_eval_pdf_var(EvalVarArgs a)
{
  math_tables_init();
  constexpr int K = Model::kParams;
  const EvalArgs& e = a.e;
  const uint64_t n4 = e.n >> 2;
  const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t < n4)
  {
    const float4 ix = ld4<true>(e.ix, t), iy = ld4<true>(e.iy, t), iz = ld4<true>(e.iz, t);
    const float4 ox = ld4<true>(e.ox, t), oy = ld4<true>(e.oy, t), oz = ld4<true>(e.oz, t);
    const uint32_t mk = e.mask ? reinterpret_cast<const uint32_t*>(e.mask)[t] : 0x01010101u;
    float4 pv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) pv[k] = a.src.vp[k] ? ld4<true>(a.src.vp[k], t) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float inx[4] = {ix.x, ix.y, ix.z, ix.w}, iny[4] = {iy.x, iy.y, iy.z, iy.w}, inz[4] = {iz.x, iz.y, iz.z, iz.w};
    const float onx[4] = {ox.x, ox.y, ox.z, ox.w}, ony[4] = {oy.x, oy.y, oy.z, oy.w}, onz[4] = {oz.x, oz.y, oz.z, oz.w};
    float r[4], g[4], b[4], p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      ParamBlock q;
#pragma unroll
      for (int k = 0; k < kMaxParams; ++k) q.v[k] = e.p.v[k];
#pragma unroll
      for (int k = 0; k < K; ++k)
      {
        const float row[4] = {pv[k].x, pv[k].y, pv[k].z, pv[k].w};
        if (a.src.vp[k]) q.v[k] = row[j];
      }
      const Model m(q.v);
      float rgb[3];
      const uint32_t comp = ((mk >> (8 * j)) & 0xffu) ? e.component : 0u;
      model_eval_pdf<MODE, EXACT>(m, mk3(inx[j], iny[j], inz[j]), mk3(onx[j], ony[j], onz[j]), comp, rgb, p[j]);
      r[j] = rgb[0]; g[j] = rgb[1]; b[j] = rgb[2];
    }
    if (MODE & kModeEval)
    {
      st4<true>(e.r, t, r[0], r[1], r[2], r[3]);
      st4<true>(e.g, t, g[0], g[1], g[2], g[3]);
      st4<true>(e.b, t, b[0], b[1], b[2], b[3]);
    }
    if (MODE & kModePdf) st4<true>(e.pdf, t, p[0], p[1], p[2], p[3]);
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x < (e.n & 3)) lane_one_pair<Model, MODE, EXACT>(a, (n4 << 2) + threadIdx.x);
}

// One pair per thread: unaligned arrays, and the rows Src::quad excludes.
template<class Model, int MODE, bool EXACT, class A>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(eval_waves<Model>::value, 8)))
void k_eval_lane1(A a)
{
  math_tables_init();
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i < eval_args_of(a.e).n) lane_one_pair<Model, MODE, EXACT>(a, i);
}

template<class Model, int S, class A>
__global__ __launch_bounds__(kBlock) void k_sample_lane(A a)
{
  math_tables_init();
  const SampleArgs& e = a.e;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= e.n) return;
  const auto l = a.src.load_lane(i);
  ParamBlock q;
  a.src.template lane_block<S>(e.p, l, i, q);
  const Model m(q.v);
  bool active = e.mask ? (e.mask[i] != 0) : true;
  active = active && a.src.lane_live(l);
  one_sample<Model>(m, e, i, active);
}

template<class Model, class A>
__global__ __launch_bounds__(kBlock) void k_refl_lane(A a)
{
  math_tables_init();
  constexpr int S = A::Src::template slots<Model>;
  const ReflArgs& e = a.e;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= e.n) return;
  const auto l = a.src.load_lane(i);
  ParamBlock q;
  a.src.template lane_block<S>(e.p, l, i, q);
  const Model m(q.v);
  float rgb[3];
  bool active = e.mask ? (e.mask[i] != 0) : true;
  active = active && a.src.lane_live(l);
  m.reflectance(mk3(e.ox[i], e.oy[i], e.oz[i]), active ? e.component : 0u, rgb);
  e.r[i] = rgb[0]; e.g[i] = rgb[1]; e.b[i] = rgb[2];
}

// a full grid of `units` threads; 0 where it exceeds the grid limit (2^31 - 1 workgroups)
inline unsigned var_blocks(uint64_t units)
{
  const uint64_t blocks = (units + kBlock - 1) / kBlock;
  return blocks > 0x7fffffffull ? 0u : unsigned(blocks < 1 ? 1 : blocks);
}

inline int var_launched(unsigned blocks)
{
  if (blocks == 0) return fail(BBM_HIP_ERR_INVALID_ARG, "batch too large for one launch");
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("kernel launch failed: ") + hipGetErrorString(err));
  return BBM_HIP_OK;
}

// What is left for the host at a launch where the kernarg block is the call's own (Src::kHostPrepare): the checks
// and derived data of the uniform launchers (launch_mode, launch_sample_mask, launch_reflectance), `params` where
// theirs run host_params.  Releases the scratch when it goes.  (A table's blocks were prepared at create.)
template<class Model>
struct LaneHost
{
  hipStream_t s;
  void* scratch = nullptr;
  int run(ParamBlock& p, uint32_t component, bool params)
  {
    if (const int rc = host_prepare<Model>::run(s)) return rc;
    if (const int rc = host_validate<Model>::run(p)) return rc;
    return params ? host_params<Model>::run(p, component, s, &scratch) : 0;
  }
  ~LaneHost() { host_params<Model>::done(scratch, s); }
};

// Whether the quad form is used for aligned arrays: the source's choice, and for the world-space table call its own
// on top of that (eval_tab_world_quad, judged per mode from the resource report; models.hpp).
template<class Model, int MODE, bool EXACT> struct eval_tab_world_quad { static constexpr bool value = true; };
// the tangent form's, judged on top of it
template<class Model, int MODE, bool EXACT> struct eval_tab_tangent_quad : eval_tab_world_quad<Model, MODE, EXACT> {};
template<class Model, int MODE, bool EXACT, class A> constexpr bool lane_quad()
{
  if constexpr (lane_tangent<A>) return A::Src::template quad<Model> && eval_tab_tangent_quad<Model, MODE, EXACT>::value;
  else if constexpr (lane_frame<A>) return A::Src::template quad<Model> && eval_tab_world_quad<Model, MODE, EXACT>::value;
  else return A::Src::template quad<Model>;
}

// The ladder: alignment -> the quad or the one-lane kernel.
template<class Model, int MODE, bool EXACT, class A>
int launch_lane_kernel(const A& a, hipStream_t s)
{
  using Src = typename A::Src;
  constexpr bool quad = lane_quad<Model, MODE, EXACT, A>();
  const EvalArgs& e = eval_args_of(a.e);
  bool vec = quad && aligned16(e.ix) && aligned16(e.iy) && aligned16(e.iz) && aligned16(e.ox) && aligned16(e.oy) &&
             aligned16(e.oz) && (reinterpret_cast<uintptr_t>(e.mask) & 3u) == 0 &&
             a.src.aligned(Src::template slots<Model>);
  if (MODE & kModeEval) vec = vec && aligned16(e.r) && aligned16(e.g) && aligned16(e.b);
  if (MODE & kModePdf) vec = vec && aligned16(e.pdf);
  if constexpr (lane_frame<A>) vec = vec && aligned16(a.e.nx) && aligned16(a.e.ny) && aligned16(a.e.nz) && aligned16(a.e.cos);
  if constexpr (lane_tangent<A>) vec = vec && aligned16(a.e.tx) && aligned16(a.e.ty) && aligned16(a.e.tz);
  const unsigned blocks = var_blocks(vec ? (e.n >> 2) : e.n);
  if (blocks == 0) return var_launched(blocks);
  if constexpr (quad)
  {
    if constexpr (std::is_same_v<A, EvalVarArgs>)
    {
      if (vec) hipLaunchKernelGGL((k_eval_pdf_var<Model, MODE, EXACT>), dim3(blocks), dim3(kBlock), 0, s, a);
    }
    else if (vec) hipLaunchKernelGGL((k_eval_lane4<Model, MODE, EXACT, A>), dim3(blocks), dim3(kBlock), 0, s, a);
  }
  if (!vec) hipLaunchKernelGGL((k_eval_lane1<Model, MODE, EXACT, A>), dim3(blocks), dim3(kBlock), 0, s, a);
  return var_launched(blocks);
}

template<class Model, class A>
int launch_sample_kernel(const A& a, hipStream_t s)
{
  const unsigned blocks = var_blocks(a.e.n);
  if (blocks == 0) return var_launched(blocks);
  constexpr int S = A::Src::template slots<Model>;
  bool twin = false;
  if constexpr (has_exact_sample<Model>())       // exact mode: the sampler's twin (launch_sample_mask)
    if (exact_on())
    {
      hipLaunchKernelGGL((k_sample_lane<exact_sample_t<Model>, S, A>), dim3(blocks), dim3(kBlock), 0, s, a);
      twin = true;
    }
  if (!twin) hipLaunchKernelGGL((k_sample_lane<Model, S, A>), dim3(blocks), dim3(kBlock), 0, s, a);
  return var_launched(blocks);
}

template<class Model, class A>
int launch_refl_kernel(const A& a, hipStream_t s)
{
  const unsigned blocks = var_blocks(a.e.n);
  if (blocks == 0) return var_launched(blocks);
  hipLaunchKernelGGL((k_refl_lane<Model, A>), dim3(blocks), dim3(kBlock), 0, s, a);
  return var_launched(blocks);
}

// Host preparation on a copy of the arguments where the source needs it, then `launch` on them.
template<class Model, class A, class Launch>
int launch_prepared(const A& a0, bool params, hipStream_t s, Launch launch)
{
  if constexpr (A::Src::kHostPrepare)
  {
    A a = a0;
    LaneHost<Model> host{s};
    if (const int rc = host.run(a.e.p, a.e.component, params)) return rc;
    return launch(a);
  }
  else return launch(a0);
}

template<class Model, int MODE, class A>
int launch_lane_exact(const A& a0, hipStream_t s)
{
  return launch_prepared<Model>(a0, (MODE & kModePdf) != 0, s, [s](const A& a) {
    if constexpr (model_has_exact<Model>())
      if (exact_on()) return launch_lane_kernel<Model, MODE, true>(a, s);
    return launch_lane_kernel<Model, MODE, false>(a, s);
  });
}

template<class Model, class A>
int launch_eval_pdf_lanes(const A& a, int mode, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    switch (mode)
    {
      case kModeEval: return launch_lane_exact<Model, kModeEval>(a, s);
      case kModePdf: return launch_lane_exact<Model, kModePdf>(a, s);
      default: return launch_lane_exact<Model, kModeEvalPdf>(a, s);
    }
  }
}

template<class Model, class A>
int launch_sample_lanes(const A& a0, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else return launch_prepared<Model>(a0, true, s, [s](const A& a) { return launch_sample_kernel<Model>(a, s); });
}

template<class Model, class A>
int launch_reflectance_lanes(const A& a0, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else return launch_prepared<Model>(a0, false, s, [s](const A& a) { return launch_refl_kernel<Model>(a, s); });
}

}  // namespace bbmhip
