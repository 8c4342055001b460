// bbm_amd/csrc/sample_eval.hpp -- one BSDF call per bounce in one launch: draw a direction for `out`, evaluate the
// model at (dir, out) and form the path's throughput weight eval . cos / pdf (bbm_hip_sample_eval and its material
// table twin bbm_hip_sample_eval_table).  Included at the end of kernels.hpp, after lanes.hpp.
//
// Lane i returns what the staged pair of calls returns for it, bit for bit: dir / pdf / flag are bbm_hip_sample's,
// value is the r, g, b of bbm_hip_eval_pdf (both outputs) at in = dir, and weight[c] is
// pdf > epsilon ? (value[c] * dir.z) / pdf : 0, the term of checkBsdf's reflectance test (k_check, kEpsF) with the
// IEEE float quotient (sample_weight).  Nothing is special-cased: a lane whose sample failed (flag 0, zero direction), a lane below the
// horizon and a masked lane evaluate the model at whatever direction the sampler returned, as the staged calls do.
// The sampled direction never leaves the registers, which is the point: 52 or 64 B per lane instead of 76.
//
// Layout: k_sample_v4's -- four consecutive lanes per thread-iteration, five 16-byte loads and one 16-byte store per
// output array, grid-stride up to max_blocks(), a scalar tail.  The mask and whether the value and the weight group
// are stored are runtime, wave-uniform arguments, so a row has one quad and one one-lane kernel, times the exact
// variant where it has one.  Unaligned arrays (and the rows sample_eval_quad excludes) take one lane per thread.
//
// FRAME (a compile-time parameter of the four kernels): the world-space calls bbm_hip_sample_eval_world and
// bbm_hip_sample_eval_table_world -- `out` and the direction in world space, one shading normal per lane, the frame
// (frame.hpp) built and applied in registers (frame_sample_eval).  Without it the kernels are the
// local calls' and hold nothing of the frame.
#pragma once

namespace bbmhip {

struct SampleEvalArgs
{
  SampleArgs s;                       // the inputs, and dir / pdf / flag (required)
  float* r; float* g; float* b;       // value = eval(dir, out); all null: not stored
  float* wr; float* wg; float* wb;    // weight; all null: not stored
  const float* nx; const float* ny; const float* nz;   // the world-space calls' shading normal per lane, else null
};
struct SampleEvalTabArgs : LaneArgs<SampleEvalArgs, TabRef> {};     // e.s.p: the fallback block (table.hpp)
// The tangent form of the world-space calls (bbm_hip_sample_eval_world_tangent and its table twin),
// for the rows whose parameters run along the frame's X and Y (anisotropic, models.hpp).  Types of their own: the
// local and normal-only kernels take SampleEvalArgs, which stays as it is.
struct SampleEvalTangentArgs : SampleEvalArgs
{
  const float* tx; const float* ty; const float* tz;   // the tangent per lane, any length
};
struct SampleEvalTabTangentArgs : LaneArgs<SampleEvalTangentArgs, TabRef> {};
template<class E> constexpr bool sample_eval_tangent = std::is_same_v<E, SampleEvalTangentArgs>;

template<class Model> constexpr bool fused_sample_eval()
{
  if constexpr (requires { Model::kFusedSampleEval; }) return Model::kFusedSampleEval;
  else return false;
}

// sample(out, xi) and eval(dir, out) of one lane.  Default mode: the model's own sample_eval where it has one (the
// microfacet models: one halfway vector and one D for both, bit-identical to the separate calls).  Exact mode
// (EXACT, a model with model_has_exact; m is then the sampler's exact twin): the sampler takes its pdf from the
// default evaluation while the staged eval runs the exact one, so the two are called one after the other -- one fused
// exact eval_pdf would return the exact pdf, which is not bbm_hip_sample's in the subnormal lanes.
template<bool EXACT, class Model>
__device__ __forceinline__ void model_sample_eval(const Model& m, v3 out, float xi0, float xi1, uint32_t comp,
                                                  v3& dir, float* rgb, float& pdf, uint32_t& flag)
{
  if constexpr (!EXACT && fused_sample_eval<Model>()) m.sample_eval(out, xi0, xi1, comp, dir, rgb, pdf, flag);
  else
  {
    float unused;
    m.sample(out, xi0, xi1, comp, dir, pdf, flag);
    model_eval_pdf<kModeEval, EXACT>(m, dir, out, comp, rgb, unused);
  }
}

// checkBsdf's importance-sampling term (checkBsdf.cpp:85-86; k_check, kCheckReflectance), per lane.  The quotient is
// the IEEE float division, as the reference's: k_check forms it with div_nr, which is that quotient except within
// ~2^-22 ulp of a rounding midpoint and -- seen on the GPU, DESIGN.md §4.16 -- where the remainder n - d q of a tiny
// normal quotient is itself subnormal (Bagher: 1.3805531e-37 for 1.3805532e-37).  Three divisions per lane of a
// kernel that moves 52-64 B per lane are not its bound.
__device__ __forceinline__ void sample_weight(const float* rgb, float dz, float pdf, float* w)
{
#pragma unroll
  for (int c = 0; c < 3; ++c) w[c] = (pdf > kEpsF) ? (rgb[c] * dz) / pdf : 0.0f;
}

// The world-space lane (FRAME; bbm_hip_sample_eval_world): `out` and the returned direction are in
// world space, the model runs in the shading frame of the lane's normal (frame.hpp), which stays in registers.
// Lane i returns what frame_to_local, the local call and frame_to_global return for it in sequence, bit for bit: a
// lane that is masked (`on` false) or whose normal is not live runs the model with component 0 at out = 0, as a
// masked lane of the local call after frame_to_local's 0, and its direction is frame_to_global's 0; `src_live`
// (a table lane's material index in range) switches the component alone, as in the local table call.  cosz is the
// local dir.z, the weight's cosine.  Without FRAME this is model_sample_eval and nothing else.
// TANGENT (with FRAME): the frame is tangent_frame(normal, tangent), the staged calls the tangent frame calls.
template<bool FRAME, bool EXACT, bool TANGENT = false, class Model>
__device__ __forceinline__ void frame_sample_eval(const Model& m, v3 normal, v3 out, float xi0, float xi1, bool on,
                                                  bool src_live, uint32_t component, v3& dir, float& cosz, float* rgb,
                                                  float& pdf, uint32_t& flag, v3 tangent = mk3(0.0f, 0.0f, 0.0f))
{
  static_assert(FRAME || !TANGENT, "a tangent belongs to a world-space call");
  if constexpr (FRAME)
  {
    const Frame f = lane_shading_frame<TANGENT>(normal, tangent);
    const bool in_frame = on && f.live;
    const v3 lo = f.to_local(out);
    v3 d;
    model_sample_eval<EXACT>(m, in_frame ? lo : mk3(0.0f, 0.0f, 0.0f), xi0, xi1,
                             (in_frame && src_live) ? component : 0u, d, rgb, pdf, flag);
    cosz = d.z;
    const v3 g = f.to_global(d);
    dir = in_frame ? g : mk3(0.0f, 0.0f, 0.0f);
  }
  else
  {
    model_sample_eval<EXACT>(m, out, xi0, xi1, (on && src_live) ? component : 0u, dir, rgb, pdf, flag);
    cosz = dir.z;
  }
}

// `on`: the lane's mask; `src_live`: see frame_sample_eval (true for the uniform call)
template<bool FRAME, bool EXACT, class Model, class E>
__device__ __forceinline__ void one_sample_eval(const Model& m, const E& a, uint64_t i, bool on, bool src_live)
{
  constexpr bool TAN = sample_eval_tangent<E>;
  const SampleArgs& s = a.s;
  v3 d; float rgb[3], pdf, cz; uint32_t f;
  const v3 nrm = FRAME ? mk3(a.nx[i], a.ny[i], a.nz[i]) : mk3(0.0f, 0.0f, 0.0f);
  v3 tan = mk3(0.0f, 0.0f, 0.0f);
  if constexpr (TAN) tan = mk3(a.tx[i], a.ty[i], a.tz[i]);
  frame_sample_eval<FRAME, EXACT, TAN>(m, nrm, mk3(s.ox[i], s.oy[i], s.oz[i]), s.xi0[i], s.xi1[i], on, src_live,
                                       s.component, d, cz, rgb, pdf, f, tan);
  s.dx[i] = d.x; s.dy[i] = d.y; s.dz[i] = d.z; s.pdf[i] = pdf; s.flag[i] = f;
  if (a.r) { a.r[i] = rgb[0]; a.g[i] = rgb[1]; a.b[i] = rgb[2]; }
  if (a.wr)
  {
    float w[3];
    sample_weight(rgb, cz, pdf, w);
    a.wr[i] = w[0]; a.wg[i] = w[1]; a.wb[i] = w[2];
  }
}

// Whether the quad form is used for aligned arrays, per mode (EXACT: the kernel the exact mode launches).  From the
// compiler's resource report: a row whose quad form has scratch where neither its k_sample_v4 nor
// its k_eval_pdf_v4 has runs one lane per thread, which for all of them needs none or less.  The uniform and the
// table kernel are judged on their own (the table's has no grid-stride loop and holds fewer registers).
// Specialised in models.hpp.
template<class Model, bool EXACT> struct sample_eval_quad { static constexpr bool value = true; };
template<class Model, bool EXACT> struct sample_eval_tab_quad { static constexpr bool value = true; };
// The world-space kernels hold the frame's nine floats across the model call, so they are judged again, on top of
// the local kernels' choice.  Specialised in models.hpp.
template<class Model, bool EXACT> struct sample_eval_world_quad : sample_eval_quad<Model, EXACT> {};
template<class Model, bool EXACT> struct sample_eval_tab_world_quad : sample_eval_tab_quad<Model, EXACT> {};
// The tangent form, judged again on top of the world kernels' choice.  Specialised in models.hpp.
template<class Model, bool EXACT> struct sample_eval_tangent_quad : sample_eval_world_quad<Model, EXACT> {};
template<class Model, bool EXACT> struct sample_eval_tab_tangent_quad : sample_eval_tab_world_quad<Model, EXACT> {};
template<bool FRAME, class Model, bool EXACT, bool TANGENT = false> constexpr bool sample_eval_use_quad()
{
  if constexpr (TANGENT) return sample_eval_tangent_quad<Model, EXACT>::value;
  else if constexpr (FRAME) return sample_eval_world_quad<Model, EXACT>::value;
  else return sample_eval_quad<Model, EXACT>::value;
}
template<bool FRAME, class Model, bool EXACT, bool TANGENT = false> constexpr bool sample_eval_tab_use_quad()
{
  if constexpr (TANGENT) return sample_eval_tab_tangent_quad<Model, EXACT>::value;
  else if constexpr (FRAME) return sample_eval_tab_world_quad<Model, EXACT>::value;
  else return sample_eval_tab_quad<Model, EXACT>::value;
}

// Occupancy: the chain is k_check's reflectance test (sample, eval, the weight), so its choice is the starting point
// (check_waves: 4 waves per SIMD, the compiler's own for the He family and EPD) -- not measured for this kernel.
#define BBM_HIP_SAMPLE_EVAL_ATTR(Model) __attribute__((amdgpu_waves_per_eu(check_waves<Model>::value, 8)))

// One quad's stores, t the quad's index in every array; the weights are formed only where they are stored.
// cz: the weight's cosine, the local dir.z (dz itself in the local kernels).
__device__ __forceinline__ void store_sample_eval(const SampleEvalArgs& a, uint64_t t, const float* dx,
                                                  const float* dy, const float* dz, const float* cz, const float* pd,
                                                  const uint32_t* fl, const float (*rgb)[4])
{
  const SampleArgs& s = a.s;
  st4<true>(s.dx, t, dx[0], dx[1], dx[2], dx[3]);
  st4<true>(s.dy, t, dy[0], dy[1], dy[2], dy[3]);
  st4<true>(s.dz, t, dz[0], dz[1], dz[2], dz[3]);
  st4<true>(s.pdf, t, pd[0], pd[1], pd[2], pd[3]);
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(u4{fl[0], fl[1], fl[2], fl[3]}, reinterpret_cast<u4*>(s.flag) + t);
  if (a.r)
  {
    st4<true>(a.r, t, rgb[0][0], rgb[0][1], rgb[0][2], rgb[0][3]);
    st4<true>(a.g, t, rgb[1][0], rgb[1][1], rgb[1][2], rgb[1][3]);
    st4<true>(a.b, t, rgb[2][0], rgb[2][1], rgb[2][2], rgb[2][3]);
  }
  if (a.wr)
  {
    float w[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const float f[3] = {rgb[0][j], rgb[1][j], rgb[2][j]};
      float wj[3];
      sample_weight(f, cz[j], pd[j], wj);
      w[0][j] = wj[0]; w[1][j] = wj[1]; w[2][j] = wj[2];
    }
    st4<true>(a.wr, t, w[0][0], w[0][1], w[0][2], w[0][3]);
    st4<true>(a.wg, t, w[1][0], w[1][1], w[1][2], w[1][3]);
    st4<true>(a.wb, t, w[2][0], w[2][1], w[2][2], w[2][3]);
  }
}

// 4 lanes per thread-iteration: 5 x 16-byte loads (out xyz, xi0, xi1), 5 + 3 + 3 x 16-byte stores.  Requires every
// array 16-byte aligned and the mask 4-byte aligned (checked on the host); the n % 4 tail runs scalar.
// FRAME: three more loads (the normal).
// E = SampleEvalTangentArgs: three more again (the tangent).
template<class Model, bool EXACT, bool FRAME, class E>
__global__ __launch_bounds__(kBlock) BBM_HIP_SAMPLE_EVAL_ATTR(Model) void k_sample_eval_v4(E a)
{
  math_tables_init();
  constexpr bool TAN = sample_eval_tangent<E>;
  const Model m(a.s.p.v);
  const SampleArgs& s = a.s;
  const uint64_t n4 = s.n >> 2;
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x; t < n4; t += stride)
  {
    const float4 ox = ld4<true>(s.ox, t), oy = ld4<true>(s.oy, t), oz = ld4<true>(s.oz, t);
    const float4 x0 = ld4<true>(s.xi0, t), x1 = ld4<true>(s.xi1, t);
    float4 wx = {}, wy = {}, wz = {};
    if constexpr (FRAME) { wx = ld4<true>(a.nx, t); wy = ld4<true>(a.ny, t); wz = ld4<true>(a.nz, t); }
    float4 tx = {}, ty = {}, tz = {};
    if constexpr (TAN) { tx = ld4<true>(a.tx, t); ty = ld4<true>(a.ty, t); tz = ld4<true>(a.tz, t); }
    const float ttx[4] = {tx.x, tx.y, tx.z, tx.w}, tty[4] = {ty.x, ty.y, ty.z, ty.w}, ttz[4] = {tz.x, tz.y, tz.z, tz.w};
    const uint32_t mk = s.mask ? reinterpret_cast<const uint32_t*>(s.mask)[t] : 0x01010101u;
    const float onx[4] = {ox.x, ox.y, ox.z, ox.w}, ony[4] = {oy.x, oy.y, oy.z, oy.w}, onz[4] = {oz.x, oz.y, oz.z, oz.w};
    const float u0[4] = {x0.x, x0.y, x0.z, x0.w}, u1[4] = {x1.x, x1.y, x1.z, x1.w};
    const float nnx[4] = {wx.x, wx.y, wx.z, wx.w}, nny[4] = {wy.x, wy.y, wy.z, wy.w}, nnz[4] = {wz.x, wz.y, wz.z, wz.w};
    float dx[4], dy[4], dz[4], cz[4], pd[4], rgb[3][4];
    uint32_t fl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      v3 d;
      float f[3];
      frame_sample_eval<FRAME, EXACT, TAN>(m, mk3(nnx[j], nny[j], nnz[j]), mk3(onx[j], ony[j], onz[j]), u0[j], u1[j],
                                           ((mk >> (8 * j)) & 0xffu) != 0, true, s.component, d, cz[j], f, pd[j], fl[j],
                                           mk3(ttx[j], tty[j], ttz[j]));
      dx[j] = d.x; dy[j] = d.y; dz[j] = d.z;
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c][j] = f[c];
    }
    store_sample_eval(a, t, dx, dy, dz, cz, pd, fl, rgb);
  }
  if (blockIdx.x == 0 && threadIdx.x < (s.n & 3))
  {
    const uint64_t i = (n4 << 2) + threadIdx.x;
    one_sample_eval<FRAME, EXACT>(m, a, i, s.mask ? (s.mask[i] != 0) : true, true);
  }
}

// Scalar path for unaligned arrays.
template<class Model, bool EXACT, bool FRAME, class E>
__global__ __launch_bounds__(kBlock) BBM_HIP_SAMPLE_EVAL_ATTR(Model) void k_sample_eval_v1(E a)
{
  math_tables_init();
  const Model m(a.s.p.v);
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < a.s.n; i += stride)
    one_sample_eval<FRAME, EXACT>(m, a, i, a.s.mask ? (a.s.mask[i] != 0) : true, true);
}

// Material tables: the same lane behind a lane-parameter source (lanes.hpp; instantiated for TabRef only, there is
// no per-row entry point).  S: the slot count of the model the table was made for (Model may be its exact-mode
// sampling twin).  One model is live at a time.
template<class Model, int S, bool EXACT, bool FRAME, class A>
__device__ __forceinline__ void lane_one_sample_eval(const A& a, uint64_t i)
{
  const SampleArgs& s = a.e.s;
  const auto l = a.src.load_lane(i);
  ParamBlock q;
  a.src.template lane_block<S>(s.p, l, i, q);
  const Model m(q.v);
  one_sample_eval<FRAME, EXACT>(m, a.e, i, s.mask ? (s.mask[i] != 0) : true, a.src.lane_live(l));
}

// Four lanes per thread; every float array and the source's own 16-byte aligned, the mask 4-byte aligned.  A full
// grid, as the other per-lane kernels.
template<class Model, int S, bool EXACT, bool FRAME, class A>
__global__ __launch_bounds__(kBlock) BBM_HIP_SAMPLE_EVAL_ATTR(Model) void k_seval_lane4(A a)
{
  math_tables_init();
  constexpr bool TAN = sample_eval_tangent<typename A::Call>;
  const SampleArgs& s = a.e.s;
  const uint64_t n4 = s.n >> 2;
  const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t < n4)
  {
    const float4 ox = ld4<true>(s.ox, t), oy = ld4<true>(s.oy, t), oz = ld4<true>(s.oz, t);
    const float4 x0 = ld4<true>(s.xi0, t), x1 = ld4<true>(s.xi1, t);
    float4 wx = {}, wy = {}, wz = {};
    if constexpr (FRAME) { wx = ld4<true>(a.e.nx, t); wy = ld4<true>(a.e.ny, t); wz = ld4<true>(a.e.nz, t); }
    float4 tx = {}, ty = {}, tz = {};
    if constexpr (TAN) { tx = ld4<true>(a.e.tx, t); ty = ld4<true>(a.e.ty, t); tz = ld4<true>(a.e.tz, t); }
    const float ttx[4] = {tx.x, tx.y, tx.z, tx.w}, tty[4] = {ty.x, ty.y, ty.z, ty.w}, ttz[4] = {tz.x, tz.y, tz.z, tz.w};
    const auto c = a.src.template load_quad<S>(t);
    const uint32_t mk = s.mask ? reinterpret_cast<const uint32_t*>(s.mask)[t] : 0x01010101u;
    const float onx[4] = {ox.x, ox.y, ox.z, ox.w}, ony[4] = {oy.x, oy.y, oy.z, oy.w}, onz[4] = {oz.x, oz.y, oz.z, oz.w};
    const float u0[4] = {x0.x, x0.y, x0.z, x0.w}, u1[4] = {x1.x, x1.y, x1.z, x1.w};
    const float nnx[4] = {wx.x, wx.y, wx.z, wx.w}, nny[4] = {wy.x, wy.y, wy.z, wy.w}, nnz[4] = {wz.x, wz.y, wz.z, wz.w};
    float dx[4], dy[4], dz[4], cz[4], pd[4], rgb[3][4];
    uint32_t fl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      ParamBlock q;
      a.src.template quad_block<S>(s.p, c, j, q);
      const Model m(q.v);
      v3 d;
      float f[3];
      frame_sample_eval<FRAME, EXACT, TAN>(m, mk3(nnx[j], nny[j], nnz[j]), mk3(onx[j], ony[j], onz[j]), u0[j], u1[j],
                                           ((mk >> (8 * j)) & 0xffu) != 0, a.src.quad_live(c, j), s.component, d, cz[j],
                                           f, pd[j], fl[j], mk3(ttx[j], tty[j], ttz[j]));
      dx[j] = d.x; dy[j] = d.y; dz[j] = d.z;
#pragma unroll
      for (int c3 = 0; c3 < 3; ++c3) rgb[c3][j] = f[c3];
    }
    store_sample_eval(a.e, t, dx, dy, dz, cz, pd, fl, rgb);
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x < (s.n & 3)) lane_one_sample_eval<Model, S, EXACT, FRAME>(a, (n4 << 2) + threadIdx.x);
}

// One lane per thread: unaligned arrays (and the rows sample_eval_tab_quad excludes).
template<class Model, int S, bool EXACT, bool FRAME, class A>
__global__ __launch_bounds__(kBlock) BBM_HIP_SAMPLE_EVAL_ATTR(Model) void k_seval_lane1(A a)
{
  math_tables_init();
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i < a.e.s.n) lane_one_sample_eval<Model, S, EXACT, FRAME>(a, i);
}

inline bool sample_eval_aligned(const SampleEvalArgs& a)
{
  const SampleArgs& s = a.s;
  return aligned16(s.ox) && aligned16(s.oy) && aligned16(s.oz) && aligned16(s.xi0) && aligned16(s.xi1) &&
         aligned16(s.dx) && aligned16(s.dy) && aligned16(s.dz) && aligned16(s.pdf) && aligned16(s.flag) &&
         aligned16(a.r) && aligned16(a.g) && aligned16(a.b) && aligned16(a.wr) && aligned16(a.wg) &&
         aligned16(a.wb) && aligned16(a.nx) && aligned16(a.ny) && aligned16(a.nz) && (reinterpret_cast<uintptr_t>(s.mask) & 3u) == 0;
}
inline bool sample_eval_aligned(const SampleEvalTangentArgs& a)
{
  return sample_eval_aligned(static_cast<const SampleEvalArgs&>(a)) && aligned16(a.tx) && aligned16(a.ty) && aligned16(a.tz);
}

// What the exact mode launches for a row: the sampler's twin where it has one (launch_sample_mask), evaluated with
// the exact eval_pdf where the model has one (launch_mode) -- the two staged calls' choices, each on its own.
template<class Model> constexpr bool sample_eval_has_exact() { return has_exact_sample<Model>() || model_has_exact<Model>(); }

// One mode's launch: K the kernels' model type (the row's, or its sampler's exact twin), QUAD the mode's trait.
template<class K, bool E, bool QUAD, bool FRAME, class Args>
void launch_sample_eval_kernel(const Args& a, hipStream_t s)
{
  const bool vec = QUAD && sample_eval_aligned(a);
  const uint64_t units = vec ? (a.s.n >> 2) : a.s.n;
  uint64_t blocks = (units + kBlock - 1) / kBlock;
  if (blocks < 1) blocks = 1;
  if (blocks > max_blocks()) blocks = max_blocks();
  if constexpr (QUAD)
  {
    if (vec) hipLaunchKernelGGL((k_sample_eval_v4<K, E, FRAME, Args>), dim3(unsigned(blocks)), dim3(kBlock), 0, s, a);
  }
  if (!vec) hipLaunchKernelGGL((k_sample_eval_v1<K, E, FRAME, Args>), dim3(unsigned(blocks)), dim3(kBlock), 0, s, a);
}

template<class Model, bool FRAME, class Args>
int launch_sample_eval_frame(const Args& a0, hipStream_t s)
{
  constexpr bool TAN = sample_eval_tangent<Args>;
  if (const int rc = host_prepare<Model>::run(s)) return rc;
  if (const int rc = host_validate<Model>::run(a0.s.p)) return rc;
  Args a = a0;
  void* scratch = nullptr;
  if (const int rc = host_params<Model>::run(a.s.p, a.s.component, s, &scratch)) return rc;
  struct Release { void* p; hipStream_t s; ~Release() { host_params<Model>::done(p, s); } } release{scratch, s};
  bool exact = false;
  if constexpr (sample_eval_has_exact<Model>())
    if (exact_on())
    {
      launch_sample_eval_kernel<exact_sample_t<Model>, model_has_exact<Model>(),
                                sample_eval_use_quad<FRAME, Model, true, TAN>(), FRAME>(a, s);
      exact = true;
    }
  if (!exact) launch_sample_eval_kernel<Model, false, sample_eval_use_quad<FRAME, Model, false, TAN>(), FRAME>(a, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("kernel launch failed: ") + hipGetErrorString(e));
  return BBM_HIP_OK;
}

// the local call, and the world-space one (a.nx / ny / nz set)
template<class Model> int launch_sample_eval(const SampleEvalArgs& a, hipStream_t s) { return launch_sample_eval_frame<Model, false>(a, s); }
template<class Model> int launch_sample_eval_world(const SampleEvalArgs& a, hipStream_t s) { return launch_sample_eval_frame<Model, true>(a, s); }
// the tangent form (a.tx / ty / tz set as well); instantiated for the anisotropic rows only
template<class Model> int launch_sample_eval_tangent(const SampleEvalTangentArgs& a, hipStream_t s) { return launch_sample_eval_frame<Model, true>(a, s); }

// a full grid, as the other per-lane kernels; 0 where the batch is too large for one launch (var_blocks)
template<class K, int S, bool E, bool QUAD, bool FRAME, class A>
unsigned launch_sample_eval_tab_kernel(const A& a, hipStream_t s)
{
  const bool vec = QUAD && sample_eval_aligned(a.e) && a.src.aligned(S);
  const unsigned blocks = var_blocks(vec ? (a.e.s.n >> 2) : a.e.s.n);
  if (blocks == 0) return blocks;
  if constexpr (QUAD)
  {
    if (vec) hipLaunchKernelGGL((k_seval_lane4<K, S, E, FRAME, A>), dim3(blocks), dim3(kBlock), 0, s, a);
  }
  if (!vec) hipLaunchKernelGGL((k_seval_lane1<K, S, E, FRAME, A>), dim3(blocks), dim3(kBlock), 0, s, a);
  return blocks;
}

// The table's blocks were prepared at create (table_prepare: host_prepare, host_validate, host_params per material),
// so, as for launch_sample_lanes, nothing is left to do on the host but choose the kernel.
template<class Model, bool FRAME, class A>
int launch_sample_eval_tab_frame(const A& a, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    constexpr bool TAN = sample_eval_tangent<typename A::Call>;
    constexpr int S = table_slots<Model>::value;
    if constexpr (sample_eval_has_exact<Model>())
      if (exact_on())
        return var_launched(launch_sample_eval_tab_kernel<exact_sample_t<Model>, S, model_has_exact<Model>(),
                                                          sample_eval_tab_use_quad<FRAME, Model, true, TAN>(), FRAME>(a, s));
    return var_launched(launch_sample_eval_tab_kernel<Model, S, false, sample_eval_tab_use_quad<FRAME, Model, false, TAN>(),
                                                      FRAME>(a, s));
  }
}

template<class Model> int launch_sample_eval_tab(const SampleEvalTabArgs& a, hipStream_t s) { return launch_sample_eval_tab_frame<Model, false>(a, s); }
template<class Model> int launch_sample_eval_tab_world(const SampleEvalTabArgs& a, hipStream_t s) { return launch_sample_eval_tab_frame<Model, true>(a, s); }
template<class Model> int launch_sample_eval_tab_tangent(const SampleEvalTabTangentArgs& a, hipStream_t s) { return launch_sample_eval_tab_frame<Model, true>(a, s); }

}  // namespace bbmhip
