// bbm_amd/csrc/varying.hpp -- per-lane model parameters: the rows source of the per-lane kernels (lanes.hpp) behind
// bbm_hip_eval_pdf_varying, bbm_hip_sample_varying and bbm_hip_reflectance_varying.  Included at
// the end of kernels.hpp.
//
// Lane i evaluates the model at q_i[k] = vp[k] ? vp[k][i] : p[k] for k < Model::kParams; every slot beyond the
// model's own parameters (EPD's gamma slots, a fused aggregate's mode slot, whatever host_params writes) is the
// uniform block's, prepared on the host exactly as for the uniform entry points.  Each lane builds its Model from
// its block and calls the device functions the uniform kernels call (model_eval_pdf, sample, reflectance), so a
// lane's result is the uniform kernel's at q_i, bit for bit.  The one exception is EPD's normalization where p
// varies: the host's tgammaf(1 / p) rides in the block tagged with the uniform p (EpdNdf), so a lane whose p has
// other bits takes the correctly rounded tgamma of the double instead, as a probe of the fitting loss does.
//
// The quad form loads one 16-byte nontemporal vector per varying row.  The fill loop is unrolled to kParams, a
// compile-time bound, so the block stays in registers; `vp[k] != nullptr` is wave-uniform.  Rows wider than
// kVarQuadParams parameters (a quad of them would not fit the register file at the model's occupancy) take one pair
// per thread.
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

// Per-parameter rows of n floats (device), nullptr = uniform: a lane-parameter source (lanes.hpp).
struct VarRows
{
  const float* vp[kMaxParams];

  // the uniform block is the call's own: host_prepare, host_validate and host_params run per launch
  static constexpr bool kHostPrepare = true;
  template<class Model> static constexpr int slots = Model::kParams;
  template<class Model> static constexpr bool quad = var_quad<Model>::value;

  bool aligned(int s) const
  {
    for (int k = 0; k < s; ++k)
      if (vp[k] && !aligned16(vp[k])) return false;
    return true;
  }

  // lane i: no state of its own, always live.  (The rows' quad form is k_eval_pdf_var in lanes.hpp, which reads vp
  // in its own body.)
  struct Lane {};
  __device__ __forceinline__ Lane load_lane(uint64_t) const { return {}; }
  template<int S> __device__ __forceinline__ void lane_block(const ParamBlock& u, Lane, uint64_t i, ParamBlock& q) const
  {
#pragma unroll
    for (int k = 0; k < kMaxParams; ++k) q.v[k] = u.v[k];
#pragma unroll
    for (int k = 0; k < S; ++k)
      if (vp[k]) q.v[k] = vp[k][i];
  }
  __device__ __forceinline__ bool lane_live(Lane) const { return true; }
};

inline int var_unsupported() { return fail(BBM_HIP_ERR_UNSUPPORTED, "this model has no per-lane parameter kernels"); }

}  // namespace bbmhip
