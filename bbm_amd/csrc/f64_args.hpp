// bbm_amd/csrc/f64_args.hpp -- the doubleRGB kernels' argument structs and launcher bundle: all the registry and
// the C-ABI need of f64.hip, without the device code of f64.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bbmhip {
namespace f64 {

constexpr int kMaxParamsF64 = 64;      // parameter block size; the last slot carries the aggregate mode (Aggregate)

struct ParamBlockF64 { double v[kMaxParamsF64]; };

struct EvalArgsF64
{
  const double* ix; const double* iy; const double* iz;
  const double* ox; const double* oy; const double* oz;
  const uint8_t* mask;
  double* r; double* g; double* b; double* pdf;
  uint64_t n;
  uint32_t component;
  ParamBlockF64 p;
};

struct ReflArgsF64
{
  const double* ox; const double* oy; const double* oz;
  const uint8_t* mask;
  double* r; double* g; double* b;
  uint64_t n;
  uint32_t component;
  ParamBlockF64 p;
};

struct SampleArgsF64
{
  const double* ox; const double* oy; const double* oz;
  const double* xi0; const double* xi1;
  const uint8_t* mask;
  double* dx; double* dy; double* dz; double* pdf; uint32_t* flag;
  uint64_t n;
  uint32_t component;
  ParamBlockF64 p;
};

using EvalLauncherF64 = int (*)(const EvalArgsF64&, hipStream_t);
using ReflLauncherF64 = int (*)(const ReflArgsF64&, hipStream_t);
using SampleLauncherF64 = int (*)(const SampleArgsF64&, hipStream_t);

// A composition's f64 launchers; all null for a model without a doubleRGB kernel.
struct F64Launchers { EvalLauncherF64 eval_pdf; ReflLauncherF64 reflectance; SampleLauncherF64 sample; };

// The doubleRGB launchers of the floatRGB composition M (models.hpp), explicitly instantiated in f64.hip for every
// composition that has_f64.
template<class M> F64Launchers f64_launchers_of();
template<class M> struct has_f64 { static constexpr bool value = true; };

}  // namespace f64
}  // namespace bbmhip
