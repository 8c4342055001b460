// bbm_amd/csrc/varying.hpp -- per-lane model parameters: the streaming kernels behind bbm_hip_eval_pdf_varying,
// bbm_hip_sample_varying and bbm_hip_reflectance_varying.  Included at the end of kernels.hpp.
//
// Lane i evaluates the model at q_i[k] = vp[k] ? vp[k][i] : p[k] for k < Model::kParams; every slot beyond the
// model's own parameters (EPD's gamma slots, a fused aggregate's mode slot, whatever host_params writes) is the
// uniform block's, prepared on the host exactly as for the uniform entry points.  Each lane builds its Model from
// its block and calls the device functions the uniform kernels call (model_eval_pdf, sample, reflectance), so a
// lane's result is the uniform kernel's at q_i, bit for bit.  The one exception is EPD's normalization where p
// varies: the host's tgammaf(1 / p) rides in the block tagged with the uniform p (EpdNdf), so a lane whose p has
// other bits takes the correctly rounded tgamma of the double instead, as a probe of the fitting loss does.
//
// Layout of the eval kernel: k_eval_pdf_v4's -- four consecutive pairs per thread, one 16-byte nontemporal load
// per direction array and per varying row, 16-byte nontemporal stores, a scalar tail -- with the model built inside
// the j loop, so one model is live at a time.  The fill loop is unrolled to Model::kParams, a compile-time bound, so
// the block stays in registers; `vp[k] != nullptr` is wave-uniform.  Rows wider than kVarQuadParams parameters (a
// quad of them would not fit the register file at the model's occupancy), and any call with an array that is not
// 16-byte aligned, take one pair per thread (k_eval_pdf_var1).  sample and reflectance run one lane per thread, as
// k_reflectance does.  All grids are full: one trip per thread, no grid-stride loop.
#pragma once

namespace bbmhip {

// Whether a composition has per-lane kernels.  Not the He family (its sample / pdf read a 90-bin CDF built per
// launch from the parameters, host_params<He<...>>: per lane that CDF does not exist) and not Merl (no parameters,
// only a table address); specialised in models.hpp.
template<class Model> struct supports_varying { static constexpr bool value = true; };

// Most parameters a row may have for the quad form of the eval kernel (from the compiler's resource report,
// the fused form of every row up to 8 parameters runs without scratch; Bagher's 30 spill 160 B)
#ifndef BBM_HIP_VAR_QUAD_PARAMS
#define BBM_HIP_VAR_QUAD_PARAMS 8
#endif
constexpr int kVarQuadParams = BBM_HIP_VAR_QUAD_PARAMS;
template<class Model> struct var_quad { static constexpr bool value = Model::kParams <= kVarQuadParams; };

// per-parameter rows of n floats (device), nullptr = uniform
struct VarRows { const float* vp[kMaxParams]; };

struct EvalVarArgs { EvalArgs e; VarRows v; };
struct SampleVarArgs { SampleArgs e; VarRows v; };
struct ReflVarArgs { ReflArgs e; VarRows v; };

// lane i's parameter block
template<class Model>
__device__ __forceinline__ void var_block(const ParamBlock& u, const VarRows& v, uint64_t i, ParamBlock& q)
{
#pragma unroll
  for (int k = 0; k < kMaxParams; ++k) q.v[k] = u.v[k];
#pragma unroll
  for (int k = 0; k < Model::kParams; ++k)
    if (v.vp[k]) q.v[k] = v.vp[k][i];
}

template<class Model, int MODE, bool EXACT>
__device__ __forceinline__ void var_one_pair(const EvalVarArgs& a, uint64_t i)
{
  const EvalArgs& e = a.e;
  ParamBlock q;
  var_block<Model>(e.p, a.v, i, q);
  const Model m(q.v);
  float rgb[3], pdf;
  const bool active = e.mask ? (e.mask[i] != 0) : true;
  model_eval_pdf<MODE, EXACT>(m, mk3(e.ix[i], e.iy[i], e.iz[i]), mk3(e.ox[i], e.oy[i], e.oz[i]),
                              active ? e.component : 0u, rgb, pdf);
  if (MODE & kModeEval) { e.r[i] = rgb[0]; e.g[i] = rgb[1]; e.b[i] = rgb[2]; }
  if (MODE & kModePdf) e.pdf[i] = pdf;
}

// Four pairs per thread; every array (varying rows included) 16-byte aligned, the mask 4-byte aligned.
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
    for (int k = 0; k < K; ++k) pv[k] = a.v.vp[k] ? ld4<true>(a.v.vp[k], t) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
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
        if (a.v.vp[k]) q.v[k] = row[j];
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
  if (blockIdx.x == 0 && threadIdx.x < (e.n & 3)) var_one_pair<Model, MODE, EXACT>(a, (n4 << 2) + threadIdx.x);
}

// One pair per thread: the wide rows (var_quad) and unaligned arrays.
template<class Model, int MODE, bool EXACT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(eval_waves<Model>::value, 8)))
void k_eval_pdf_var1(EvalVarArgs a)
{
  math_tables_init();
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i < a.e.n) var_one_pair<Model, MODE, EXACT>(a, i);
}

template<class Model>
__global__ __launch_bounds__(kBlock) void k_sample_var(SampleVarArgs a)
{
  math_tables_init();
  const SampleArgs& e = a.e;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= e.n) return;
  ParamBlock q;
  var_block<Model>(e.p, a.v, i, q);
  const Model m(q.v);
  one_sample<Model>(m, e, i, e.mask ? (e.mask[i] != 0) : true);
}

template<class Model>
__global__ __launch_bounds__(kBlock) void k_reflectance_var(ReflVarArgs a)
{
  math_tables_init();
  const ReflArgs& e = a.e;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= e.n) return;
  ParamBlock q;
  var_block<Model>(e.p, a.v, i, q);
  const Model m(q.v);
  float rgb[3];
  const bool active = e.mask ? (e.mask[i] != 0) : true;
  m.reflectance(mk3(e.ox[i], e.oy[i], e.oz[i]), active ? e.component : 0u, rgb);
  e.r[i] = rgb[0]; e.g[i] = rgb[1]; e.b[i] = rgb[2];
}

inline int var_unsupported() { return fail(BBM_HIP_ERR_UNSUPPORTED, "this model has no per-lane parameter kernels"); }

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

inline bool var_rows_aligned16(const VarRows& v, int nparams)
{
  for (int k = 0; k < nparams; ++k)
    if (v.vp[k] && !aligned16(v.vp[k])) return false;
  return true;
}

template<class Model, int MODE, bool EXACT>
int launch_var_mode(const EvalVarArgs& a0, hipStream_t s)
{
  if (const int rc = host_prepare<Model>::run(s)) return rc;
  if (const int rc = host_validate<Model>::run(a0.e.p)) return rc;
  EvalVarArgs a = a0;
  void* scratch = nullptr;
  if (MODE & kModePdf)
    if (const int rc = host_params<Model>::run(a.e.p, a.e.component, s, &scratch)) return rc;
  struct Release { void* p; hipStream_t s; ~Release() { host_params<Model>::done(p, s); } } release{scratch, s};
  const EvalArgs& e = a.e;
  bool vec = var_quad<Model>::value && aligned16(e.ix) && aligned16(e.iy) && aligned16(e.iz) && aligned16(e.ox) &&
             aligned16(e.oy) && aligned16(e.oz) && (reinterpret_cast<uintptr_t>(e.mask) & 3u) == 0 &&
             var_rows_aligned16(a.v, Model::kParams);
  if (MODE & kModeEval) vec = vec && aligned16(e.r) && aligned16(e.g) && aligned16(e.b);
  if (MODE & kModePdf) vec = vec && aligned16(e.pdf);
  const unsigned blocks = var_blocks(vec ? (e.n >> 2) : e.n);
  if (blocks == 0) return var_launched(blocks);
  if constexpr (var_quad<Model>::value)
  {
    if (vec) hipLaunchKernelGGL((k_eval_pdf_var<Model, MODE, EXACT>), dim3(blocks), dim3(kBlock), 0, s, a);
  }
  if (!vec) hipLaunchKernelGGL((k_eval_pdf_var1<Model, MODE, EXACT>), dim3(blocks), dim3(kBlock), 0, s, a);
  return var_launched(blocks);
}

template<class Model, int MODE>
int launch_var_exact(const EvalVarArgs& a, hipStream_t s)
{
  if constexpr (model_has_exact<Model>())
    if (exact_on()) return launch_var_mode<Model, MODE, true>(a, s);
  return launch_var_mode<Model, MODE, false>(a, s);
}

template<class Model>
int launch_eval_pdf_var(const EvalVarArgs& a, int mode, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    switch (mode)
    {
      case kModeEval: return launch_var_exact<Model, kModeEval>(a, s);
      case kModePdf: return launch_var_exact<Model, kModePdf>(a, s);
      default: return launch_var_exact<Model, kModeEvalPdf>(a, s);
    }
  }
}

template<class Model>
int launch_sample_var(const SampleVarArgs& a0, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    if (const int rc = host_prepare<Model>::run(s)) return rc;
    if (const int rc = host_validate<Model>::run(a0.e.p)) return rc;
    SampleVarArgs a = a0;
    void* scratch = nullptr;
    if (const int rc = host_params<Model>::run(a.e.p, a.e.component, s, &scratch)) return rc;
    struct Release { void* p; hipStream_t s; ~Release() { host_params<Model>::done(p, s); } } release{scratch, s};
    const unsigned blocks = var_blocks(a.e.n);
    if (blocks == 0) return var_launched(blocks);
    bool twin = false;
    if constexpr (has_exact_sample<Model>())       // exact mode: the sampler's twin (launch_sample_mask)
      if (exact_on())
      {
        hipLaunchKernelGGL((k_sample_var<exact_sample_t<Model>>), dim3(blocks), dim3(kBlock), 0, s, a);
        twin = true;
      }
    if (!twin) hipLaunchKernelGGL((k_sample_var<Model>), dim3(blocks), dim3(kBlock), 0, s, a);
    return var_launched(blocks);
  }
}

template<class Model>
int launch_reflectance_var(const ReflVarArgs& a, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    if (const int rc = host_prepare<Model>::run(s)) return rc;
    if (const int rc = host_validate<Model>::run(a.e.p)) return rc;
    const unsigned blocks = var_blocks(a.e.n);
    if (blocks == 0) return var_launched(blocks);
    hipLaunchKernelGGL((k_reflectance_var<Model>), dim3(blocks), dim3(kBlock), 0, s, a);
    return var_launched(blocks);
  }
}

}  // namespace bbmhip
