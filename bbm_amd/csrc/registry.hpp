// bbm_amd/csrc/registry.hpp -- what the C-ABI (bbm_hip.hip) sees of the model registry (registry.hip): a row by
// id, with its launcher bundles and parameter count.
#pragma once
#include "kernels.hpp"
#include "f64_args.hpp"

namespace bbmhip {

struct ModelEntry
{
  const char* name;
  int nparams;
  uint32_t components;
  Launchers run;                 // floatRGB
  f64::F64Launchers run_f64;     // doubleRGB; all null where the composition has none (f64::has_f64)
  // attributes in declaration order (bbm::reflection::attributes, the order toString prints and parameter_values
  // packs), "name:count" with count = product of the attribute's shape; nullptr: not constructible from a string
  const char* layout;
  float defaults[kMaxParams];
  float lower[kMaxParams];
  float upper[kMaxParams];
  // per-parameter bsdf_attr flags (include/bbm/bsdf_attr_flag.h:16-29), one letter per parameter:
  // d DiffuseScale, D DiffuseParameter, s SpecularScale, p SpecularParameter, x Dependent
  const char* attrs;
  TangentLaunchers tangent;      // all null but for the anisotropic rows (bbm_hip_model_anisotropic)
};

// a registry id, or a fused aggregate's id with BBM_HIP_RUNTIME_AGGREGATE (its aggregatebsdf semantics)
bool runtime_id(int id);
// the row of a model id (BBM_HIP_RUNTIME_AGGREGATE / BBM_HIP_CALL_* bits allowed), or nullptr
const ModelEntry* entry(int id);
// What every per-model call checks first, in this order: the id, for a doubleRGB call (f64) that the model has
// doubleRGB kernels, the parameter count, and with check_params the parameter pointer.
int checked_entry(int model_id, int nparams, const void* params, bool check_params, bool f64, const ModelEntry*& e);

}  // namespace bbmhip
