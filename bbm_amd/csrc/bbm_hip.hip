// bbm_amd/csrc/bbm_hip.hip -- libbbm_hip.so: the per-model calls of the C-ABI declared in include/bbm_hip.h, the
// synthetic direction generator and the other small utility kernels with their entry points.  The model kernels
// live in kernels.hpp and are instantiated per family in inst_*.hip; the rows that name them are in registry.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/bbm_hip.h"
#include "registry.hpp"
#include "aggregate.hpp"  // kAggregateModeSlot
#include "merl.hpp"       // bbm_hip_merl_table
#include "set.hpp"        // the material sets' plan, gather and scatter launchers

namespace bbmhip {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg)
{
  g_last_error = msg;
  return code;
}

int launched(const char* what)
{
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return BBM_HIP_OK;
  return fail(BBM_HIP_ERR_HIP, std::string(what ? what : "kernel launch failed") + ": " + hipGetErrorString(e));
}

int epd_table_host(float* out, int capacity);

namespace {

static_assert(kAggregateModeSlot == kMaxParams - 1, "the aggregate mode travels in the parameter block's last slot");

int prepare(int model_id, const float* params, int nparams, size_t n, EvalArgs& a, const ModelEntry*& e)
{
  if (const int rc = checked_entry(model_id, nparams, params, true, false, e)) return rc;
  std::memset(&a, 0, sizeof(a));
  for (int i = 0; i < nparams; ++i) a.p.v[i] = params[i];
  a.p.v[kAggregateModeSlot] = runtime_id(model_id) ? 1.0f : 0.0f;
  a.n = n;
  return BBM_HIP_OK;
}

int check_dirs(const float* x, const float* y, const float* z, const char* what)
{
  if (!x || !y || !z) return fail(BBM_HIP_ERR_INVALID_ARG, std::string(what) + " direction pointer is NULL");
  return BBM_HIP_OK;
}

// ------------------------------------------------------------------- synthetic directions

// Counter-based generator: splitmix64 finaliser over (seed, stream, index).  Two 24-bit uniforms
// per direction.  Pure function of the global index -> shards regenerate identical slices.
__global__ __launch_bounds__(kBlock) void k_fill_dirs(uint64_t key, uint64_t offset, uint64_t n, int mode,
                                                       float* __restrict__ x, float* __restrict__ y, float* __restrict__ z)
{
  math_tables_init();
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
  {
    const uint64_t h = mix64(key + 0x9e3779b97f4a7c15ull * (offset + i));
    const float u1 = float(uint32_t(h >> 40)) * (1.0f / 16777216.0f);
    const float u2 = float(uint32_t(h >> 16) & 0xffffffu) * (1.0f / 16777216.0f);
    const float zz = (mode == 0) ? u1 : 2.0f * u1 - 1.0f;
    const float s = sqrtf(fmaxf(1.0f - zz * zz, 0.0f));
    float sp, cp;
    sincosf(2.0f * kPiF * u2, &sp, &cp);
    x[i] = s * cp;
    y[i] = s * sp;
    z[i] = zz;
  }
}

__global__ __launch_bounds__(kBlock) void k_linearize(LinDesc d, uint64_t begin, uint64_t n, float* __restrict__ ix,
                                                      float* __restrict__ iy, float* __restrict__ iz, float* __restrict__ ox,
                                                      float* __restrict__ oy, float* __restrict__ oz)
{
  math_tables_init();
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
  {
    v3 in, out;
    lin_pair(d, begin + i, in, out);
    ix[i] = in.x; iy[i] = in.y; iz[i] = in.z;
    ox[i] = out.x; oy[i] = out.y; oz[i] = out.z;
  }
}

int to_desc(const bbm_hip_linearizer* lin, LinDesc& d)
{
  if (!lin) return fail(BBM_HIP_ERR_INVALID_ARG, "linearizer is NULL");
  if (lin->kind != kLinSpherical && lin->kind != kLinMerl)
    return fail(BBM_HIP_ERR_INVALID_ARG, "linearizer kind must be BBM_LIN_SPHERICAL or BBM_LIN_MERL");
  std::memset(&d, 0, sizeof(d));
  d.kind = lin->kind;
  for (int k = 0; k < 2; ++k)
  {
    if (lin->samples_in[k] == 0 || lin->samples_out[k] == 0)
      return fail(BBM_HIP_ERR_INVALID_ARG, "linearizer sample counts must be positive");
    d.s_in[k] = lin->samples_in[k];
    d.s_out[k] = lin->samples_out[k];
    d.start_in[k] = lin->start_in[k];
    d.start_out[k] = lin->start_out[k];
    d.size_in[k] = lin->end_in[k] - lin->start_in[k];      // _sizeIn(endIn - startIn), float
    d.size_out[k] = lin->end_out[k] - lin->start_out[k];
  }
  return BBM_HIP_OK;
}

}  // namespace

__global__ __launch_bounds__(kBlock) void k_loss_final(const double* block_sums, int nblocks, int nprobes, double* sums)
{
  math_tables_init();
  __shared__ double part[kBlock];
  const int p = blockIdx.x;
  double t = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += kBlock) t += block_sums[size_t(b) * nprobes + p];
  part[threadIdx.x] = t;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1)
  {
    if (int(threadIdx.x) < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[p] = part[0];
}

// partials [slot][b][kCheckAcc] -> acc[slot][kCheckAcc]: one wave per slot, fixed order
__global__ __launch_bounds__(64) void k_check_final(const double* partial, int nblocks, double* acc)
{
  math_tables_init();
  const int slot = blockIdx.x;
  double r[kCheckAcc];
#pragma unroll
  for (int e = 0; e < kCheckAcc; ++e) r[e] = 0.0;
  r[kCheckSums] = r[kCheckSums + 2] = -1.0;
  r[kCheckSums + 1] = r[kCheckSums + 3] = 1.8e19;
  for (int b = threadIdx.x; b < nblocks; b += 64)
  {
    const double* p = partial + (size_t(slot) * nblocks + b) * kCheckAcc;
#pragma unroll
    for (int e = 0; e < kCheckSums; ++e) r[e] += p[e];
    max_pair(r[kCheckSums], r[kCheckSums + 1], p[kCheckSums], p[kCheckSums + 1]);
    max_pair(r[kCheckSums + 2], r[kCheckSums + 3], p[kCheckSums + 2], p[kCheckSums + 3]);
  }
  wave_reduce_check(r);
  if (threadIdx.x == 0)
  {
#pragma unroll
    for (int e = 0; e < kCheckAcc; ++e) acc[size_t(slot) * kCheckAcc + e] = r[e];
  }
}

namespace {

// draw k of a check test: base key of the stream (test, k); the slot is mixed in by check_key

__global__ __launch_bounds__(kBlock) void k_draws(uint64_t key, uint64_t offset, uint64_t n, float* u0, float* u1)
{
  math_tables_init();
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
    uniform2(key, offset + i, u0[i], u1[i]);
}

__global__ __launch_bounds__(kBlock) void k_trials(uint64_t base, int ntrials, int sphere, float* x, float* y, float* z)
{
  math_tables_init();
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= ntrials) return;
  float u0, u1;
  uniform2(check_key(base, t), 0, u0, u1);
  const v3 d = sphere_dir(u0, u1, sphere == 0);
  x[t] = d.x; y[t] = d.y; z[t] = d.z;
}

__global__ __launch_bounds__(kBlock) void k_sphere_dirs(const float* u0, const float* u1, uint64_t n, int hemisphere,
                                                        float* x, float* y, float* z)
{
  math_tables_init();
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
  {
    const v3 d = sphere_dir(u0[i], u1[i], hemisphere != 0);
    x[i] = d.x; y[i] = d.y; z[i] = d.z;
  }
}

// bbm_hip_libm_eval: the device's restated libm floats, elementwise
__global__ __launch_bounds__(kBlock) void k_libm(int func, const float* a, const float* b, float* out, uint64_t n)
{
  math_tables_init();
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride)
  {
    const float x = a[i];
    float r;
    switch (func)
    {
      case BBM_HIP_LIBM_EXPF: r = expf_glibc(x); break;
      case BBM_HIP_LIBM_LOGF: r = logf_glibc(x); break;
      case BBM_HIP_LIBM_POWF: r = powf_glibc(x, b[i]); break;
      case BBM_HIP_LIBM_ERFF: r = erff_glibc(x); break;
      case BBM_HIP_LIBM_ONE_PLUS_SQRT: r = f_one_plus_sqrt(1.0 + double(x) * double(b[i])); break;
      case BBM_HIP_LIBM_SINF: { float c; sincosf_glibc(x, &r, &c); } break;
      case BBM_HIP_LIBM_COSF: { float sn; sincosf_glibc(x, &sn, &r); } break;
      case BBM_HIP_LIBM_ATAN2F: r = atan2f_glibc(x, b[i]); break;
      case BBM_HIP_LIBM_THETA: r = theta_of(mk3(x, 0.0f, b[i])); break;
      default: r = erfcf_glibc(x); break;
    }
    out[i] = r;
  }
}

}  // namespace

}  // namespace bbmhip

using namespace bbmhip;

namespace {

// The pointer checks a family of entry points shares once the model (or table) is known, and the argument block
// filled from them; the parameter block `p` is the caller's to set.

// mode: the uniform calls' explicit mode, whose outputs are then required; 0 from the varying and table calls, which
// take it from the outputs that are not NULL.
int eval_args(int& mode, const float* in_x, const float* in_y, const float* in_z,
              const float* out_x, const float* out_y, const float* out_z, const uint8_t* mask, size_t n,
              uint32_t component, float* r, float* g, float* b, float* pdf, EvalArgs& a)
{
  int rc;
  if ((rc = check_dirs(in_x, in_y, in_z, "in")) || (rc = check_dirs(out_x, out_y, out_z, "out"))) return rc;
  if (mode)
  {
    if ((mode & kModeEval) && (!r || !g || !b)) return fail(BBM_HIP_ERR_INVALID_ARG, "eval output pointer is NULL");
    if ((mode & kModePdf) && !pdf) return fail(BBM_HIP_ERR_INVALID_ARG, "pdf output pointer is NULL");
  }
  else
  {
    const bool want_eval = r || g || b;
    if (want_eval && (!r || !g || !b)) return fail(BBM_HIP_ERR_INVALID_ARG, "eval output pointer is NULL");
    if (!want_eval && !pdf) return fail(BBM_HIP_ERR_INVALID_ARG, "every output pointer is NULL");
    mode = (want_eval ? kModeEval : 0) | (pdf ? kModePdf : 0);
  }
  std::memset(&a, 0, sizeof(a));
  a.n = n;
  a.ix = in_x; a.iy = in_y; a.iz = in_z; a.ox = out_x; a.oy = out_y; a.oz = out_z;
  a.mask = mask; a.r = r; a.g = g; a.b = b; a.pdf = pdf;
  a.component = component & kFlagAll;
  return BBM_HIP_OK;
}

int sample_args(const float* out_x, const float* out_y, const float* out_z, const float* xi0, const float* xi1,
                const uint8_t* mask, size_t n, uint32_t component,
                float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag, SampleArgs& a)
{
  if (const int rc = check_dirs(out_x, out_y, out_z, "out")) return rc;
  if (!xi0 || !xi1) return fail(BBM_HIP_ERR_INVALID_ARG, "xi pointer is NULL");
  if (!dir_x || !dir_y || !dir_z || !pdf || !flag) return fail(BBM_HIP_ERR_INVALID_ARG, "sample output pointer is NULL");
  std::memset(&a, 0, sizeof(a));
  a.n = n;
  a.ox = out_x; a.oy = out_y; a.oz = out_z; a.xi0 = xi0; a.xi1 = xi1; a.mask = mask;
  a.dx = dir_x; a.dy = dir_y; a.dz = dir_z; a.pdf = pdf; a.flag = flag;
  a.component = component & kFlagAll;
  return BBM_HIP_OK;
}

// sample_args, and a value or weight group that is all three pointers or none
int sample_eval_args(const float* out_x, const float* out_y, const float* out_z, const float* xi0, const float* xi1,
                     const uint8_t* mask, size_t n, uint32_t component,
                     float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                     float* r, float* g, float* b, float* wr, float* wg, float* wb, SampleEvalArgs& a)
{
  if (const int rc = sample_args(out_x, out_y, out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, a.s))
    return rc;
  if ((r || g || b) && (!r || !g || !b)) return fail(BBM_HIP_ERR_INVALID_ARG, "value output: give r, g and b or none");
  if ((wr || wg || wb) && (!wr || !wg || !wb))
    return fail(BBM_HIP_ERR_INVALID_ARG, "weight output: give wr, wg and wb or none");
  a.r = r; a.g = g; a.b = b; a.wr = wr; a.wg = wg; a.wb = wb;
  a.nx = a.ny = a.nz = nullptr;        // the world-space calls set them
  return BBM_HIP_OK;
}

// The tangent of the *_tangent calls: all three pointers (the tangent call), none (the call is its counterpart
// without one); a mixture is an error, found before anything else is looked at.
int tangent_arg(const float* tx, const float* ty, const float* tz, bool& tangent)
{
  tangent = tx && ty && tz;
  if (!tangent && (tx || ty || tz)) return fail(BBM_HIP_ERR_INVALID_ARG, "tangent: give tx, ty and tz or none");
  return BBM_HIP_OK;
}

int refl_args(const float* out_x, const float* out_y, const float* out_z, const uint8_t* mask, size_t n,
              uint32_t component, float* r, float* g, float* b, ReflArgs& a)
{
  if (const int rc = check_dirs(out_x, out_y, out_z, "out")) return rc;
  if (!r || !g || !b) return fail(BBM_HIP_ERR_INVALID_ARG, "reflectance output pointer is NULL");
  std::memset(&a, 0, sizeof(a));
  a.n = n;
  a.ox = out_x; a.oy = out_y; a.oz = out_z; a.mask = mask; a.r = r; a.g = g; a.b = b;
  a.component = component & kFlagAll;
  return BBM_HIP_OK;
}

}  // namespace

extern "C" {

int bbm_hip_abi_version(void) { return BBM_HIP_ABI_VERSION; }

int bbm_hip_set_exact_subnormals(int on) { return exact_subnormals().exchange(on != 0 ? 1 : 0); }

const char* bbm_hip_last_error(void) { return g_last_error.c_str(); }

static int eval_common(int mode, int model_id, const float* params, int nparams,
                       const float* in_x, const float* in_y, const float* in_z,
                       const float* out_x, const float* out_y, const float* out_z,
                       const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                       float* r, float* g, float* b, float* pdf, void* stream)
{
  (void)unit;   // no model on this path depends on unit_t (bsdfmodel/microfacet.h:74, lambertian.h:45)
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp, a;
  const ModelEntry* e;
  int rc = prepare(model_id, params, nparams, n, tmp, e);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if ((rc = eval_args(mode, in_x, in_y, in_z, out_x, out_y, out_z, mask, n, component, r, g, b, pdf, a))) return rc;
  a.p = tmp.p;
  return e->run.eval_pdf(a, mode, static_cast<hipStream_t>(stream));
}

int bbm_hip_eval(int model_id, const float* params, int nparams,
                 const float* in_x, const float* in_y, const float* in_z,
                 const float* out_x, const float* out_y, const float* out_z,
                 const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                 float* r, float* g, float* b, void* stream)
{
  return eval_common(kModeEval, model_id, params, nparams, in_x, in_y, in_z, out_x, out_y, out_z, mask, n,
                     component, unit, r, g, b, nullptr, stream);
}

int bbm_hip_pdf(int model_id, const float* params, int nparams,
                const float* in_x, const float* in_y, const float* in_z,
                const float* out_x, const float* out_y, const float* out_z,
                const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                float* pdf, void* stream)
{
  return eval_common(kModePdf, model_id, params, nparams, in_x, in_y, in_z, out_x, out_y, out_z, mask, n,
                     component, unit, nullptr, nullptr, nullptr, pdf, stream);
}

int bbm_hip_eval_pdf(int model_id, const float* params, int nparams,
                     const float* in_x, const float* in_y, const float* in_z,
                     const float* out_x, const float* out_y, const float* out_z,
                     const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                     float* r, float* g, float* b, float* pdf, void* stream)
{
  return eval_common(kModeEvalPdf, model_id, params, nparams, in_x, in_y, in_z, out_x, out_y, out_z, mask, n,
                     component, unit, r, g, b, pdf, stream);
}

int bbm_hip_sample(int model_id, const float* params, int nparams,
                   const float* out_x, const float* out_y, const float* out_z,
                   const float* xi0, const float* xi1,
                   const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                   float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                   void* stream)
{
  (void)unit;
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  const ModelEntry* e;
  int rc = prepare(model_id, params, nparams, n, tmp, e);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  SampleArgs a;
  if ((rc = sample_args(out_x, out_y, out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, a)))
    return rc;
  a.p = tmp.p;
  return e->run.sample(a, static_cast<hipStream_t>(stream));
}

// world: the normal pointers are the call's (bbm_hip_sample_eval_world), else they are not looked at; the tangent
// pointers (bbm_hip_sample_eval_world_tangent) are all set or all NULL, and read only by an anisotropic row
static int sample_eval_common(bool world, int model_id, const float* params, int nparams,
                              const float* nx, const float* ny, const float* nz,
                              const float* tx, const float* ty, const float* tz,
                              const float* out_x, const float* out_y, const float* out_z,
                              const float* xi0, const float* xi1,
                              const uint8_t* mask, size_t n, uint32_t component,
                              float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                              float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  const ModelEntry* e;
  int rc = prepare(model_id, params, nparams, n, tmp, e);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if (world && (rc = check_dirs(nx, ny, nz, "normal"))) return rc;
  SampleEvalArgs a;
  if ((rc = sample_eval_args(out_x, out_y, out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag,
                             r, g, b, wr, wg, wb, a)))
    return rc;
  a.s.p = tmp.p;
  if (!world) return e->run.sample_eval(a, static_cast<hipStream_t>(stream));
  a.nx = nx; a.ny = ny; a.nz = nz;
  if (tx && e->tangent.sample_eval)
  {
    SampleEvalTangentArgs t;
    static_cast<SampleEvalArgs&>(t) = a;
    t.tx = tx; t.ty = ty; t.tz = tz;
    return e->tangent.sample_eval(t, static_cast<hipStream_t>(stream));
  }
  return e->run.sample_eval_world(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_sample_eval(int model_id, const float* params, int nparams,
                        const float* out_x, const float* out_y, const float* out_z,
                        const float* xi0, const float* xi1,
                        const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                        float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                        float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  return sample_eval_common(false, model_id, params, nparams, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            out_x, out_y, out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, r, g, b,
                            wr, wg, wb, stream);
}

int bbm_hip_sample_eval_world(int model_id, const float* params, int nparams,
                              const float* nx, const float* ny, const float* nz,
                              const float* out_x, const float* out_y, const float* out_z,
                              const float* xi0, const float* xi1,
                              const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                              float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                              float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  return sample_eval_common(true, model_id, params, nparams, nx, ny, nz, nullptr, nullptr, nullptr, out_x, out_y, out_z,
                            xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, r, g, b, wr, wg, wb, stream);
}

int bbm_hip_sample_eval_world_tangent(int model_id, const float* params, int nparams,
                                      const float* nx, const float* ny, const float* nz,
                                      const float* tx, const float* ty, const float* tz,
                                      const float* out_x, const float* out_y, const float* out_z,
                                      const float* xi0, const float* xi1,
                                      const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                      float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                                      float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  bool tangent;
  if (const int rc = tangent_arg(tx, ty, tz, tangent)) return rc;
  return sample_eval_common(true, model_id, params, nparams, nx, ny, nz, tx, ty, tz, out_x, out_y, out_z,
                            xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, r, g, b, wr, wg, wb, stream);
}

// eval / pdf / eval + pdf in world space (eval_world.hpp).  The mode is taken from the outputs that are not NULL, with
// bbm_hip_eval_pdf_varying's checks (eval_args); the normal is required, the cosine optional.
// tx, ty, tz: all set (bbm_hip_eval_pdf_world_tangent) or all NULL; read only by an anisotropic row
static int eval_pdf_world_common(int model_id, const float* params, int nparams,
                                 const float* nx, const float* ny, const float* nz,
                                 const float* tx, const float* ty, const float* tz,
                                 const float* in_x, const float* in_y, const float* in_z,
                                 const float* out_x, const float* out_y, const float* out_z,
                                 const uint8_t* mask, size_t n, uint32_t component,
                                 float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  const ModelEntry* e;
  int rc = prepare(model_id, params, nparams, n, tmp, e);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if ((rc = check_dirs(nx, ny, nz, "normal"))) return rc;
  EvalWorldArgs a;
  int mode = 0;
  if ((rc = eval_args(mode, in_x, in_y, in_z, out_x, out_y, out_z, mask, n, component, r, g, b, pdf, a.e))) return rc;
  a.e.p = tmp.p;
  a.nx = nx; a.ny = ny; a.nz = nz; a.cos = cos_in;
  if (tx && e->tangent.eval_pdf)
  {
    EvalTangentArgs t;
    static_cast<EvalWorldArgs&>(t) = a;
    t.tx = tx; t.ty = ty; t.tz = tz;
    return e->tangent.eval_pdf(t, mode, static_cast<hipStream_t>(stream));
  }
  return e->run.eval_pdf_world(a, mode, static_cast<hipStream_t>(stream));
}

int bbm_hip_eval_pdf_world(int model_id, const float* params, int nparams,
                           const float* nx, const float* ny, const float* nz,
                           const float* in_x, const float* in_y, const float* in_z,
                           const float* out_x, const float* out_y, const float* out_z,
                           const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                           float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  (void)unit;
  return eval_pdf_world_common(model_id, params, nparams, nx, ny, nz, nullptr, nullptr, nullptr, in_x, in_y, in_z,
                               out_x, out_y, out_z, mask, n, component, r, g, b, pdf, cos_in, stream);
}

int bbm_hip_eval_pdf_world_tangent(int model_id, const float* params, int nparams,
                                   const float* nx, const float* ny, const float* nz,
                                   const float* tx, const float* ty, const float* tz,
                                   const float* in_x, const float* in_y, const float* in_z,
                                   const float* out_x, const float* out_y, const float* out_z,
                                   const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                   float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  (void)unit;
  bool tangent;
  if (const int rc = tangent_arg(tx, ty, tz, tangent)) return rc;
  return eval_pdf_world_common(model_id, params, nparams, nx, ny, nz, tx, ty, tz, in_x, in_y, in_z,
                               out_x, out_y, out_z, mask, n, component, r, g, b, pdf, cos_in, stream);
}

// ------------------------------------------------------------------------------- shading frames (frame.hpp)

static int frame_common(bool to_local, const float* nx, const float* ny, const float* nz,
                        const float* tx, const float* ty, const float* tz, const float* x, const float* y, const float* z, const uint8_t* mask, size_t n,
                        float* rx, float* ry, float* rz, void* stream)
{
  if (n == 0) return BBM_HIP_OK;
  int rc;
  if ((rc = check_dirs(nx, ny, nz, "normal")) || (rc = check_dirs(x, y, z, "input")) ||
      (rc = check_dirs(rx, ry, rz, "output")))
    return rc;
  const FrameArgs a{nx, ny, nz, x, y, z, mask, n, rx, ry, rz};
  if (!tx) return frame_launch(a, to_local, static_cast<hipStream_t>(stream));
  FrameTangentArgs t;
  static_cast<FrameArgs&>(t) = a;
  t.tx = tx; t.ty = ty; t.tz = tz;
  return frame_launch(t, to_local, static_cast<hipStream_t>(stream));
}

int bbm_hip_frame_to_local(const float* nx, const float* ny, const float* nz,
                           const float* x, const float* y, const float* z, const uint8_t* mask, size_t n,
                           float* lx, float* ly, float* lz, void* stream)
{
  return frame_common(true, nx, ny, nz, nullptr, nullptr, nullptr, x, y, z, mask, n, lx, ly, lz, stream);
}

int bbm_hip_frame_to_global(const float* nx, const float* ny, const float* nz,
                            const float* lx, const float* ly, const float* lz, const uint8_t* mask, size_t n,
                            float* x, float* y, float* z, void* stream)
{
  return frame_common(false, nx, ny, nz, nullptr, nullptr, nullptr, lx, ly, lz, mask, n, x, y, z, stream);
}

int bbm_hip_frame_to_local_tangent(const float* nx, const float* ny, const float* nz,
                                   const float* tx, const float* ty, const float* tz,
                                   const float* x, const float* y, const float* z, const uint8_t* mask, size_t n,
                                   float* lx, float* ly, float* lz, void* stream)
{
  bool tangent;
  if (const int rc = tangent_arg(tx, ty, tz, tangent)) return rc;
  return frame_common(true, nx, ny, nz, tx, ty, tz, x, y, z, mask, n, lx, ly, lz, stream);
}

int bbm_hip_frame_to_global_tangent(const float* nx, const float* ny, const float* nz,
                                    const float* tx, const float* ty, const float* tz,
                                    const float* lx, const float* ly, const float* lz, const uint8_t* mask, size_t n,
                                    float* x, float* y, float* z, void* stream)
{
  bool tangent;
  if (const int rc = tangent_arg(tx, ty, tz, tangent)) return rc;
  return frame_common(false, nx, ny, nz, tx, ty, tz, lx, ly, lz, mask, n, x, y, z, stream);
}

int bbm_hip_reflectance(int model_id, const float* params, int nparams,
                        const float* out_x, const float* out_y, const float* out_z,
                        const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                        float* r, float* g, float* b, void* stream)
{
  (void)unit;
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  const ModelEntry* e;
  int rc = prepare(model_id, params, nparams, n, tmp, e);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  ReflArgs a;
  if ((rc = refl_args(out_x, out_y, out_z, mask, n, component, r, g, b, a))) return rc;
  a.p = tmp.p;
  return e->run.reflectance(a, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------- per-lane parameters (varying.hpp)

// What the three per-lane calls check first, in checked_entry's order: the id, that the row has per-lane kernels, the
// parameter count and pointer; then the uniform block (prepare) and the rows.
static int prepare_var(int model_id, const float* params, int nparams, const float* const* varying, size_t n,
                       EvalArgs& a, VarRows& v, const ModelEntry*& e)
{
  e = entry(model_id);
  if (e && !e->run.eval_pdf_var)
    return fail(BBM_HIP_ERR_UNSUPPORTED, std::string(e->name) + ": no per-lane parameter kernels");
  if (const int rc = prepare(model_id, params, nparams, n, a, e)) return rc;
  std::memset(&v, 0, sizeof(v));
  for (int k = 0; varying && k < nparams; ++k) v.vp[k] = varying[k];
  return BBM_HIP_OK;
}

int bbm_hip_eval_pdf_varying(int model_id, const float* params, int nparams, const float* const* varying,
                             const float* in_x, const float* in_y, const float* in_z,
                             const float* out_x, const float* out_y, const float* out_z,
                             const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                             float* r, float* g, float* b, float* pdf, void* stream)
{
  (void)unit;
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  EvalVarArgs a;
  const ModelEntry* e;
  int rc = prepare_var(model_id, params, nparams, varying, n, tmp, a.src, e);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  int mode = 0;
  if ((rc = eval_args(mode, in_x, in_y, in_z, out_x, out_y, out_z, mask, n, component, r, g, b, pdf, a.e))) return rc;
  a.e.p = tmp.p;
  return e->run.eval_pdf_var(a, mode, static_cast<hipStream_t>(stream));
}

int bbm_hip_sample_varying(int model_id, const float* params, int nparams, const float* const* varying,
                           const float* out_x, const float* out_y, const float* out_z,
                           const float* xi0, const float* xi1,
                           const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                           float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag, void* stream)
{
  (void)unit;
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  SampleVarArgs a;
  const ModelEntry* e;
  int rc = prepare_var(model_id, params, nparams, varying, n, tmp, a.src, e);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if ((rc = sample_args(out_x, out_y, out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, a.e)))
    return rc;
  a.e.p = tmp.p;
  return e->run.sample_var(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_reflectance_varying(int model_id, const float* params, int nparams, const float* const* varying,
                                const float* out_x, const float* out_y, const float* out_z,
                                const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                float* r, float* g, float* b, void* stream)
{
  (void)unit;
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  ReflVarArgs a;
  const ModelEntry* e;
  int rc = prepare_var(model_id, params, nparams, varying, n, tmp, a.src, e);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if ((rc = refl_args(out_x, out_y, out_z, mask, n, component, r, g, b, a.e))) return rc;
  a.e.p = tmp.p;
  return e->run.reflectance_var(a, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------- material tables (table.hpp)

}  // extern "C"

// One model's parameter sets as prepared blocks in device memory (table.hpp).  `raw` is what eval alone and
// reflectance read, `prepared` what eval + pdf, pdf and sample read (host_params applied); one allocation where the
// two are equal, which is every row but EPD.  first_*: material 0's blocks, the kernarg fallback of a lane whose
// index is out of range, with the aggregate mode slot of the id given to create.
struct bbm_hip_table
{
  int model_id;
  const ModelEntry* e;
  uint32_t count;
  float* raw;
  float* prepared;
  ParamBlock first_raw, first_prepared;
};

namespace {

int table_call(const bbm_hip_table* t, int call_flags, size_t n, const uint32_t* material)
{
  if (!t) return fail(BBM_HIP_ERR_INVALID_ARG, "table is NULL");
  if ((call_flags & ~(BBM_HIP_CALL_EXACT | BBM_HIP_CALL_DEFAULT)) != 0 ||
      call_flags == (BBM_HIP_CALL_EXACT | BBM_HIP_CALL_DEFAULT))
    return fail(BBM_HIP_ERR_INVALID_ARG, "call_flags must be 0, BBM_HIP_CALL_EXACT or BBM_HIP_CALL_DEFAULT");
  if (n > 0 && !material) return fail(BBM_HIP_ERR_INVALID_ARG, "material index pointer is NULL");
  return BBM_HIP_OK;
}

}  // namespace

extern "C" {

int bbm_hip_table_create(int model_id, const float* params, int nparams, uint32_t nmaterials, void* stream,
                         bbm_hip_table** out)
{
  const ModelEntry* e = entry(model_id);
  if (e && !e->run.eval_pdf_tab)
    return fail(BBM_HIP_ERR_UNSUPPORTED, std::string(e->name) + ": no material-table kernels");
  if (const int rc = checked_entry(model_id, nparams, params, false, false, e)) return rc;
  if (model_id & (BBM_HIP_CALL_EXACT | BBM_HIP_CALL_DEFAULT))
    return fail(BBM_HIP_ERR_INVALID_ARG, "BBM_HIP_CALL_* belongs to the batch calls' call_flags, not to a table's model id");
  if (!params) return fail(BBM_HIP_ERR_INVALID_ARG, "params is NULL");
  if (nmaterials == 0) return fail(BBM_HIP_ERR_INVALID_ARG, "a table needs at least one material");
  if (!out) return fail(BBM_HIP_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  std::unique_ptr<bbm_hip_table> t(new bbm_hip_table{model_id, e, nmaterials, nullptr, nullptr, {}, {}});
  std::vector<float> raw, prepared;
  size_t stride = 0;
  bool same = true;
  for (uint32_t m = 0; m < nmaterials; ++m)
  {
    ParamBlock in;
    std::memset(&in, 0, sizeof(in));
    for (int k = 0; k < nparams; ++k) in.v[k] = params[size_t(m) * size_t(nparams) + size_t(k)];
    in.v[kAggregateModeSlot] = runtime_id(model_id) ? 1.0f : 0.0f;
    TableBlocks b;
    if (const int rc = e->run.table_prepare(in, m == 0, s, b)) return rc;
    if (m == 0)
    {
      stride = size_t(table_stride(b.slots));
      raw.assign(size_t(nmaterials) * stride, 0.0f);
      prepared.assign(size_t(nmaterials) * stride, 0.0f);
      t->first_raw = b.raw;
      t->first_prepared = b.prepared;
    }
    std::memcpy(&raw[size_t(m) * stride], b.raw.v, size_t(b.slots) * sizeof(float));
    std::memcpy(&prepared[size_t(m) * stride], b.prepared.v, size_t(b.slots) * sizeof(float));
    same = same && std::memcmp(b.raw.v, b.prepared.v, size_t(b.slots) * sizeof(float)) == 0;
  }
  // upload in stream order; the host copies are released once the stream has taken them
  const size_t bytes = raw.size() * sizeof(float);
  const auto upload = [&](const std::vector<float>& h, float*& d) {
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (err == hipSuccess) err = hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, s);
    return err;
  };
  hipError_t err = upload(prepared, t->prepared);
  if (err == hipSuccess && !same) err = upload(raw, t->raw);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  if (err != hipSuccess)
  {
    (void)hipGetLastError();
    if (t->raw) (void)hipFree(t->raw);
    if (t->prepared) (void)hipFree(t->prepared);
    return fail(BBM_HIP_ERR_HIP, std::string("material table upload failed: ") + hipGetErrorString(err));
  }
  if (same) t->raw = t->prepared;
  *out = t.release();
  return BBM_HIP_OK;
}

int bbm_hip_table_destroy(bbm_hip_table* t)
{
  if (!t) return BBM_HIP_OK;
  // hipFree waits for the device, so launches already enqueued on the table finish first
  hipError_t err = hipFree(t->prepared);
  if (t->raw != t->prepared)
  {
    const hipError_t err2 = hipFree(t->raw);
    if (err == hipSuccess) err = err2;
  }
  delete t;
  if (err != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("hipFree failed: ") + hipGetErrorString(err));
  return BBM_HIP_OK;
}

int bbm_hip_table_model(const bbm_hip_table* t)
{
  return t ? t->model_id : fail(BBM_HIP_ERR_INVALID_ARG, "table is NULL");
}

uint32_t bbm_hip_table_size(const bbm_hip_table* t) { return t ? t->count : 0u; }

int bbm_hip_eval_pdf_table(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                           const float* in_x, const float* in_y, const float* in_z,
                           const float* out_x, const float* out_y, const float* out_z,
                           const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                           float* r, float* g, float* b, float* pdf, void* stream)
{
  (void)unit;
  int rc = table_call(t, call_flags, n, material);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  const CallExactScope mode_scope(call_flags);
  EvalTabArgs a;
  int mode = 0;
  if ((rc = eval_args(mode, in_x, in_y, in_z, out_x, out_y, out_z, mask, n, component, r, g, b, pdf, a.e))) return rc;
  // host_params runs for the uniform call only where a pdf is asked for (launch_mode)
  a.e.p = (mode & kModePdf) ? t->first_prepared : t->first_raw;
  a.src = {(mode & kModePdf) ? t->prepared : t->raw, material, t->count};
  return t->e->run.eval_pdf_tab(a, mode, static_cast<hipStream_t>(stream));
}

static int eval_pdf_table_world_common(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                                       const float* nx, const float* ny, const float* nz,
                                       const float* tx, const float* ty, const float* tz,
                                       const float* in_x, const float* in_y, const float* in_z,
                                       const float* out_x, const float* out_y, const float* out_z,
                                       const uint8_t* mask, size_t n, uint32_t component,
                                       float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  int rc = table_call(t, call_flags, n, material);
  if (rc) return rc;
  if (!t->e->run.eval_pdf_tab_world)
    return fail(BBM_HIP_ERR_UNSUPPORTED, std::string(t->e->name) + ": no material-table kernels");
  if (n == 0) return BBM_HIP_OK;
  if ((rc = check_dirs(nx, ny, nz, "normal"))) return rc;
  const CallExactScope mode_scope(call_flags);
  EvalTabWorldArgs a;
  int mode = 0;
  if ((rc = eval_args(mode, in_x, in_y, in_z, out_x, out_y, out_z, mask, n, component, r, g, b, pdf, a.e.e))) return rc;
  // the block form the local call reads (bbm_hip_eval_pdf_table)
  a.e.e.p = (mode & kModePdf) ? t->first_prepared : t->first_raw;
  a.e.nx = nx; a.e.ny = ny; a.e.nz = nz; a.e.cos = cos_in;
  a.src = {(mode & kModePdf) ? t->prepared : t->raw, material, t->count};
  if (tx && t->e->tangent.eval_pdf_tab)
  {
    EvalTabTangentArgs ta;
    static_cast<EvalWorldArgs&>(ta.e) = a.e;
    ta.e.tx = tx; ta.e.ty = ty; ta.e.tz = tz;
    ta.src = a.src;
    return t->e->tangent.eval_pdf_tab(ta, mode, static_cast<hipStream_t>(stream));
  }
  return t->e->run.eval_pdf_tab_world(a, mode, static_cast<hipStream_t>(stream));
}

int bbm_hip_eval_pdf_table_world(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                                 const float* nx, const float* ny, const float* nz,
                                 const float* in_x, const float* in_y, const float* in_z,
                                 const float* out_x, const float* out_y, const float* out_z,
                                 const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                 float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  (void)unit;
  return eval_pdf_table_world_common(t, call_flags, material, nx, ny, nz, nullptr, nullptr, nullptr, in_x, in_y, in_z,
                                     out_x, out_y, out_z, mask, n, component, r, g, b, pdf, cos_in, stream);
}

int bbm_hip_eval_pdf_table_world_tangent(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                                         const float* nx, const float* ny, const float* nz,
                                         const float* tx, const float* ty, const float* tz,
                                         const float* in_x, const float* in_y, const float* in_z,
                                         const float* out_x, const float* out_y, const float* out_z,
                                         const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                         float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  (void)unit;
  bool tangent;
  if (const int rc = tangent_arg(tx, ty, tz, tangent)) return rc;
  return eval_pdf_table_world_common(t, call_flags, material, nx, ny, nz, tx, ty, tz, in_x, in_y, in_z,
                                     out_x, out_y, out_z, mask, n, component, r, g, b, pdf, cos_in, stream);
}

int bbm_hip_sample_table(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                         const float* out_x, const float* out_y, const float* out_z,
                         const float* xi0, const float* xi1,
                         const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                         float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag, void* stream)
{
  (void)unit;
  int rc = table_call(t, call_flags, n, material);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  const CallExactScope mode_scope(call_flags);
  SampleTabArgs a;
  if ((rc = sample_args(out_x, out_y, out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, a.e)))
    return rc;
  a.e.p = t->first_prepared;
  a.src = {t->prepared, material, t->count};
  return t->e->run.sample_tab(a, static_cast<hipStream_t>(stream));
}

static int sample_eval_table_common(bool world, const bbm_hip_table* t, int call_flags, const uint32_t* material,
                                    const float* nx, const float* ny, const float* nz,
                                    const float* tx, const float* ty, const float* tz,
                                    const float* out_x, const float* out_y, const float* out_z,
                                    const float* xi0, const float* xi1,
                                    const uint8_t* mask, size_t n, uint32_t component,
                                    float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                                    float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  int rc = table_call(t, call_flags, n, material);
  if (rc) return rc;
  if (!t->e->run.sample_eval_tab)
    return fail(BBM_HIP_ERR_UNSUPPORTED, std::string(t->e->name) + ": no material-table kernels");
  if (n == 0) return BBM_HIP_OK;
  if (world && (rc = check_dirs(nx, ny, nz, "normal"))) return rc;
  const CallExactScope mode_scope(call_flags);
  SampleEvalTabArgs a;
  if ((rc = sample_eval_args(out_x, out_y, out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag,
                             r, g, b, wr, wg, wb, a.e)))
    return rc;
  // the block form sample and eval + pdf read (host_params applied)
  a.e.s.p = t->first_prepared;
  a.src = {t->prepared, material, t->count};
  if (!world) return t->e->run.sample_eval_tab(a, static_cast<hipStream_t>(stream));
  a.e.nx = nx; a.e.ny = ny; a.e.nz = nz;
  if (tx && t->e->tangent.sample_eval_tab)
  {
    SampleEvalTabTangentArgs ta;
    static_cast<SampleEvalArgs&>(ta.e) = a.e;
    ta.e.tx = tx; ta.e.ty = ty; ta.e.tz = tz;
    ta.src = a.src;
    return t->e->tangent.sample_eval_tab(ta, static_cast<hipStream_t>(stream));
  }
  return t->e->run.sample_eval_tab_world(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_sample_eval_table(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                              const float* out_x, const float* out_y, const float* out_z,
                              const float* xi0, const float* xi1,
                              const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                              float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                              float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  return sample_eval_table_common(false, t, call_flags, material, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  out_x, out_y, out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag,
                                  r, g, b, wr, wg, wb, stream);
}

int bbm_hip_sample_eval_table_world(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                                    const float* nx, const float* ny, const float* nz,
                                    const float* out_x, const float* out_y, const float* out_z,
                                    const float* xi0, const float* xi1,
                                    const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                    float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                                    float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  return sample_eval_table_common(true, t, call_flags, material, nx, ny, nz, nullptr, nullptr, nullptr, out_x, out_y,
                                  out_z, xi0, xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, r, g, b, wr, wg,
                                  wb, stream);
}

int bbm_hip_sample_eval_table_world_tangent(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                                            const float* nx, const float* ny, const float* nz,
                                            const float* tx, const float* ty, const float* tz,
                                            const float* out_x, const float* out_y, const float* out_z,
                                            const float* xi0, const float* xi1,
                                            const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                            float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                                            float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  bool tangent;
  if (const int rc = tangent_arg(tx, ty, tz, tangent)) return rc;
  return sample_eval_table_common(true, t, call_flags, material, nx, ny, nz, tx, ty, tz, out_x, out_y, out_z, xi0, xi1,
                                  mask, n, component, dir_x, dir_y, dir_z, pdf, flag, r, g, b, wr, wg, wb, stream);
}

int bbm_hip_reflectance_table(const bbm_hip_table* t, int call_flags, const uint32_t* material,
                              const float* out_x, const float* out_y, const float* out_z,
                              const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                              float* r, float* g, float* b, void* stream)
{
  (void)unit;
  int rc = table_call(t, call_flags, n, material);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  const CallExactScope mode_scope(call_flags);
  ReflTabArgs a;
  if ((rc = refl_args(out_x, out_y, out_z, mask, n, component, r, g, b, a.e))) return rc;
  a.e.p = t->first_raw;
  a.src = {t->raw, material, t->count};
  return t->e->run.reflectance_tab(a, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------- material sets (set.hpp)

}  // extern "C"

// An ordered list of tables addressed by one global id per lane: table k owns [rows.off[k], rows.off[k + 1]).
struct bbm_hip_set
{
  std::vector<const bbm_hip_table*> tables;
  SetRows rows;
};

// The stable partition of n lanes by table.  src and local are one device allocation of 2 x slots uint32; seg is the
// host copy of the segment starts (seg[rows] = capacity <= slots).  compact: the lanes whose id is out of range are in
// no slot (bbm_hip_set_plan_create_compact).
struct bbm_hip_set_plan
{
  const bbm_hip_set* set;
  uint32_t n, slots;
  bool compact;
  uint32_t* src;
  uint32_t* local;
  uint32_t seg[kSetMaxRows + 1];
};

namespace {

// The streams of a call, in lane order or in slot order.  tan: tx, ty, tz, all or none.  in: nx, ny, nz (all: the world
// call; none: the local call), then in and out (eval + pdf) or out, xi0 and xi1 (sample_eval).  res: r, g, b, pdf and
// cos_in, or dir, pdf, flag (a four-byte stream like the rest), r, g, b, wr, wg and wb.

// What every call on a plan checks first, in this order: the tangent's mixture, the plan, the call flags, the length,
// the normal's mixture, a tangent without a normal.  lanes: a call in lane order, whose `count` is the plan's n and
// which refuses a compact plan before anything else about it (it scatters through src, which would leave a dropped
// lane's outputs unwritten); otherwise a call in plan order, whose `count` is the plan's capacity.  done: nothing is
// left to do (no lane, no slot), found before any stream but the tangent is looked at.
int set_call(const bbm_hip_set_plan* p, bool lanes, int call_flags, size_t count, const float* const* tan,
             const float* const* in, bool& world, bool& done)
{
  bool tangent;
  done = world = false;
  if (const int rc = tangent_arg(tan[0], tan[1], tan[2], tangent)) return rc;
  if (lanes && p && p->compact)
    return fail(BBM_HIP_ERR_INVALID_ARG, "a compact plan leaves lanes out: use the calls in plan order (the *_sorted calls)");
  if (!p) return fail(BBM_HIP_ERR_INVALID_ARG, "plan is NULL");
  if (const int rc = table_call(p->set->tables[0], call_flags, 0, nullptr)) return rc;
  const size_t have = lanes ? p->n : p->seg[p->set->rows.rows];
  if (count != have)
    return fail(BBM_HIP_ERR_INVALID_ARG,
                lanes ? "n is " + std::to_string(count) + ", the plan was made for " + std::to_string(have) + " lanes"
                      : "slots is " + std::to_string(count) + ", the plan's capacity is " + std::to_string(have));
  if ((done = have == 0)) return BBM_HIP_OK;
  world = in[0] && in[1] && in[2];
  if (!world && (in[0] || in[1] || in[2])) return fail(BBM_HIP_ERR_INVALID_ARG, "normal: give nx, ny and nz or none");
  if (tangent && !world) return fail(BBM_HIP_ERR_INVALID_ARG, "tangent needs a normal: it fills the frame of the world-space call");
  return BBM_HIP_OK;
}

// Everything eval + pdf checks before its first launch, in either order.
int set_eval_pdf_check(const bbm_hip_set_plan* p, bool lanes, int call_flags, const float* const* tan,
                       const float* const* in, const uint8_t* mask, size_t count, uint32_t component,
                       float* const* res, bool& world, bool& done)
{
  int rc = set_call(p, lanes, call_flags, count, tan, in, world, done);
  if (rc || done) return rc;
  if (res[4] && !world) return fail(BBM_HIP_ERR_INVALID_ARG, "cos_in needs a normal: it is the cosine of `in` against it");
  EvalArgs checked;
  int mode = 0;
  if ((rc = eval_args(mode, in[3], in[4], in[5], in[6], in[7], in[8], mask, count, component, res[0], res[1], res[2],
                      res[3], checked)))
    return rc;
  for (const bbm_hip_table* t : p->set->tables)
    if (world && !t->e->run.eval_pdf_tab_world)
      return fail(BBM_HIP_ERR_UNSUPPORTED, std::string(t->e->name) + ": no material-table kernels");
  return BBM_HIP_OK;
}

// The same for sample_eval.
int set_sample_eval_check(const bbm_hip_set_plan* p, bool lanes, int call_flags, const float* const* tan,
                          const float* const* in, const uint8_t* mask, size_t count, uint32_t component,
                          float* const* res, bool& world, bool& done)
{
  int rc = set_call(p, lanes, call_flags, count, tan, in, world, done);
  if (rc || done) return rc;
  SampleEvalArgs checked;
  if ((rc = sample_eval_args(in[3], in[4], in[5], in[6], in[7], mask, count, component, res[0], res[1], res[2], res[3],
                             reinterpret_cast<uint32_t*>(res[4]), res[5], res[6], res[7], res[8], res[9], res[10],
                             checked)))
    return rc;
  for (const bbm_hip_table* t : p->set->tables)
    if (!t->e->run.sample_eval_tab || (world && !t->e->run.sample_eval_tab_world))
      return fail(BBM_HIP_ERR_UNSUPPORTED, std::string(t->e->name) + ": no material-table kernels");
  return BBM_HIP_OK;
}

// slot o of a stream in slot order; a stream that is not given stays NULL
template<class T> T* at(T* p, size_t o) { return p ? p + o : nullptr; }

// The row loop of a call kind: the table call on every segment of the plan that has slots.  The streams are in slot
// order: the caller's own (the *_sorted calls) or the scratch of a call in lane order (set_lane_order).
using SetRowLoop = int(const bbm_hip_set_plan& plan, int call_flags, bool world, const float* const* tan,
                       const float* const* in, const uint8_t* mask, uint32_t component, uint32_t unit,
                       float* const* res, void* stream);

int set_eval_pdf_rows(const bbm_hip_set_plan& plan, int call_flags, bool world, const float* const* tan,
                      const float* const* in, const uint8_t* mask, uint32_t component, uint32_t unit,
                      float* const* res, void* stream)
{
  for (uint32_t k = 0; k < plan.set->rows.rows; ++k)
  {
    const size_t o = plan.seg[k], nk = plan.seg[k + 1] - o;
    if (nk == 0) continue;
    const bbm_hip_table* t = plan.set->tables[k];
    const float *tk[3], *i[9];
    float* r[5];
    for (int c = 0; c < 3; ++c) tk[c] = at(tan[c], o);
    for (int c = 0; c < 9; ++c) i[c] = at(in[c], o);
    for (int c = 0; c < 5; ++c) r[c] = at(res[c], o);
    const int rc =
        world ? eval_pdf_table_world_common(t, call_flags, plan.local + o, i[0], i[1], i[2], tk[0], tk[1], tk[2], i[3],
                                            i[4], i[5], i[6], i[7], i[8], at(mask, o), nk, component, r[0], r[1], r[2],
                                            r[3], r[4], stream)
              : bbm_hip_eval_pdf_table(t, call_flags, plan.local + o, i[3], i[4], i[5], i[6], i[7], i[8], at(mask, o),
                                       nk, component, unit, r[0], r[1], r[2], r[3], stream);
    if (rc) return rc;
  }
  return BBM_HIP_OK;
}

int set_sample_eval_rows(const bbm_hip_set_plan& plan, int call_flags, bool world, const float* const* tan,
                         const float* const* in, const uint8_t* mask, uint32_t component, uint32_t,
                         float* const* res, void* stream)
{
  for (uint32_t k = 0; k < plan.set->rows.rows; ++k)
  {
    const size_t o = plan.seg[k], nk = plan.seg[k + 1] - o;
    if (nk == 0) continue;
    const bbm_hip_table* t = plan.set->tables[k];
    const float *tk[3], *i[8];
    float* r[11];
    for (int c = 0; c < 3; ++c) tk[c] = at(tan[c], o);
    for (int c = 0; c < 8; ++c) i[c] = at(in[c], o);
    for (int c = 0; c < 11; ++c) r[c] = at(res[c], o);
    uint32_t* flag = reinterpret_cast<uint32_t*>(r[4]);
    const int rc =
        world ? sample_eval_table_common(true, t, call_flags, plan.local + o, i[0], i[1], i[2], tk[0], tk[1], tk[2],
                                         i[3], i[4], i[5], i[6], i[7], at(mask, o), nk, component, r[0], r[1], r[2],
                                         r[3], flag, r[5], r[6], r[7], r[8], r[9], r[10], stream)
              : bbm_hip_sample_eval_table(t, call_flags, plan.local + o, i[3], i[4], i[5], i[6], i[7], at(mask, o), nk,
                                          component, 0u, r[0], r[1], r[2], r[3], flag, r[5], r[6], r[7], r[8], r[9],
                                          r[10], stream);
    if (rc) return rc;
  }
  return BBM_HIP_OK;
}

// a plan's move with no stream in it yet
SetMoveArgs set_move(const bbm_hip_set_plan& p)
{
  SetMoveArgs m;
  std::memset(&m, 0, sizeof(m));
  m.src = p.src; m.n = p.n; m.capacity = p.seg[p.set->rows.rows];
  return m;
}

// a caller stream and its sorted twin, entered into a gather (lane -> slot) or a scatter (slot -> lane)
void move_in(SetMoveArgs& m, const void* lanes, void* sorted)
{
  m.from[m.count] = static_cast<const uint32_t*>(lanes);
  m.to[m.count++] = static_cast<uint32_t*>(sorted);
}
void move_out(SetMoveArgs& m, void* sorted, void* lanes)
{
  m.from[m.count] = static_cast<const uint32_t*>(sorted);
  m.to[m.count++] = static_cast<uint32_t*>(lanes);
}

// The sorted buffers of a call in lane order: `streams` arrays of capacity four-byte slots and the mask bytes, one
// scratch block.  A take past the block yields NULL and makes status() an error, which the call returns before its
// first launch: a count that disagrees with the takes never becomes a write outside the block.
struct SetScratch
{
  char* base = nullptr;
  size_t used = 0, size = 0, stride = 0;
  hipStream_t s = nullptr;
  int acquire(uint32_t capacity, int streams, bool mask, hipStream_t stream)
  {
    s = stream;
    stride = size_t(capacity) * 4u;
    size = stride * size_t(streams) + (mask ? capacity : 0u);
    base = static_cast<char*>(scratch_acquire(size, s));
    return base ? BBM_HIP_OK : fail(BBM_HIP_ERR_HIP, "material set scratch: " + scratch_failure());
  }
  template<class T> T* take(size_t bytes)
  {
    T* p = used + bytes <= size ? reinterpret_cast<T*>(base + used) : nullptr;
    used += bytes;
    return p;
  }
  // The sorted twins of the streams of lanes[] that are given, which a move holds in this order: each goes to the
  // move's slot-order `side` (a gather's to, a scatter's from) and to slot[c], which is NULL where lanes[c] is.
  template<class L, class P> void twins(L* const* lanes, int count, P* side, float** slot)
  {
    for (int c = 0, j = 0; c < count; ++c)
    {
      slot[c] = lanes[c] ? take<float>(stride) : nullptr;
      if (lanes[c]) side[j++] = reinterpret_cast<uint32_t*>(slot[c]);
    }
  }
  int status() const
  {
    return used <= size ? BBM_HIP_OK : fail(BBM_HIP_ERR_HIP, "material set scratch: more streams taken than entered");
  }
  ~SetScratch() { if (base) scratch_release(base, s); }
};

// whether a row of the set reads a tangent (bbm_hip_model_anisotropic)
bool set_any_anisotropic(const bbm_hip_set& set)
{
  for (const bbm_hip_table* t : set.tables)
    if (t->e->tangent.eval_pdf_tab) return true;
  return false;
}

// A call in lane order: the call in plan order, `rows`, between a gather of the nin + 3 input
// streams into scratch and a scatter of the nout output streams out of it.  The streams that are given enter the
// moves, which counts them; the block is acquired for that many, and their twins are then taken from it in the order
// of entry: gathered, scattered, tangent, mask.
int set_lane_order(SetRowLoop* rows, const bbm_hip_set_plan& plan, int call_flags, bool world, const float* const* tan,
                   const float* const* lanes, int nin, const uint8_t* mask, uint32_t component, uint32_t unit,
                   float* const* res, int nout, void* stream)
{
  const hipStream_t s = static_cast<hipStream_t>(stream);
  // The tangent's gather is a launch of its own (k_set_gather carries kSetMaxIn streams, which normal, in and out
  // fill); without an anisotropic row the tangent is neither gathered nor passed on.
  const float* const none[3] = {};
  if (!set_any_anisotropic(*plan.set)) tan = none;
  SetMoveArgs in = set_move(plan), out = in, tan_in = in;
  for (int c = 0; c < nin; ++c)
    if (lanes[c]) move_in(in, lanes[c], nullptr);
  for (int c = 0; c < nout; ++c)
    if (res[c]) move_out(out, nullptr, res[c]);
  for (int c = 0; c < 3; ++c)
    if (tan[c]) move_in(tan_in, tan[c], nullptr);
  SetScratch scratch;
  int rc = scratch.acquire(in.capacity, in.count + out.count + tan_in.count, mask != nullptr, s);
  if (rc) return rc;
  float *sorted[kSetMaxIn], *sres[kSetMaxOut], *stan[3];
  scratch.twins(lanes, nin, in.to, sorted);
  scratch.twins(res, nout, out.from, sres);
  scratch.twins(tan, 3, tan_in.to, stan);
  in.mask_from = mask;
  in.mask_to = mask ? scratch.take<uint8_t>(in.capacity) : nullptr;
  if ((rc = scratch.status()) || (rc = set_gather_launch(in, s))) return rc;
  if (tan_in.count && (rc = set_gather_launch(tan_in, s))) return rc;
  if ((rc = rows(plan, call_flags, world, stan, sorted, in.mask_to, component, unit, sres, stream))) return rc;
  return set_scatter_launch(out, s);
}

}  // namespace

extern "C" {

int bbm_hip_set_create(const bbm_hip_table* const* tables, uint32_t ntables, bbm_hip_set** out)
{
  if (!tables) return fail(BBM_HIP_ERR_INVALID_ARG, "tables is NULL");
  if (ntables == 0 || ntables > kSetMaxRows)
    return fail(BBM_HIP_ERR_INVALID_ARG, "a material set holds 1 to 32 tables, got " + std::to_string(ntables));
  if (!out) return fail(BBM_HIP_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  uint64_t total = 0;
  for (uint32_t k = 0; k < ntables; ++k)
  {
    if (!tables[k]) return fail(BBM_HIP_ERR_INVALID_ARG, "table " + std::to_string(k) + " is NULL");
    total += tables[k]->count;
  }
  if (total >= 0xFFFFFFFFull)
    return fail(BBM_HIP_ERR_INVALID_ARG, "a material set holds fewer than 2^32 - 1 materials, got " + std::to_string(total));
  std::unique_ptr<bbm_hip_set> s(new bbm_hip_set);
  std::memset(&s->rows, 0, sizeof(s->rows));
  s->rows.rows = ntables;
  for (uint32_t k = 0; k < ntables; ++k)
  {
    s->tables.push_back(tables[k]);
    s->rows.off[k + 1] = s->rows.off[k] + tables[k]->count;
  }
  *out = s.release();
  return BBM_HIP_OK;
}

int bbm_hip_set_destroy(bbm_hip_set* set)
{
  delete set;      // a set owns no device memory: its offsets travel in the kernarg
  return BBM_HIP_OK;
}

uint32_t bbm_hip_set_size(const bbm_hip_set* set) { return set ? set->rows.off[set->rows.rows] : 0u; }

uint32_t bbm_hip_set_rows(const bbm_hip_set* set) { return set ? set->rows.rows : 0u; }

uint32_t bbm_hip_set_offset(const bbm_hip_set* set, uint32_t k)
{
  return set && k <= set->rows.rows ? set->rows.off[k] : 0xFFFFFFFFu;
}

int bbm_hip_set_plan_geometry(uint32_t* tile, uint32_t* scan_chunk)
{
  if (tile) *tile = kSetTile;
  if (scan_chunk) *scan_chunk = kSetScanChunk;
  return BBM_HIP_OK;
}

static int set_plan_create_common(const bbm_hip_set* set, const uint32_t* material, size_t n, void* stream,
                                  bbm_hip_set_plan** out, bool drop)
{
  if (!set) return fail(BBM_HIP_ERR_INVALID_ARG, "set is NULL");
  if (!out) return fail(BBM_HIP_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  if (n > 0 && !material) return fail(BBM_HIP_ERR_INVALID_ARG, "material index pointer is NULL");
  const uint32_t rows = set->rows.rows;
  if (uint64_t(n) + 4ull * rows + 4ull >= 0xFFFFFFFFull)
    return fail(BBM_HIP_ERR_INVALID_ARG, "batch too large for one plan");
  std::unique_ptr<bbm_hip_set_plan> p(new bbm_hip_set_plan);
  std::memset(p.get(), 0, sizeof(*p));
  p->set = set;
  p->n = uint32_t(n);
  p->compact = drop;
  if (n == 0)
  {
    *out = p.release();
    return BBM_HIP_OK;
  }
  const hipStream_t s = static_cast<hipStream_t>(stream);
  p->slots = ((p->n + 3u) & ~3u) + 4u * rows;
  SetPlanArgs a;
  std::memset(&a, 0, sizeof(a));
  a.rows = set->rows;
  a.material = material;
  a.n = p->n;
  a.groups = (p->n + kSetTile - 1) / kSetTile;
  a.slots = p->slots;
  a.drop = drop ? 1u : 0u;
  hipError_t err = hipMalloc(reinterpret_cast<void**>(&p->src), size_t(p->slots) * 8u);
  if (err != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(BBM_HIP_ERR_HIP, std::string("material plan allocation failed: ") + hipGetErrorString(err));
  }
  p->local = p->src + p->slots;
  a.src = p->src;
  a.local = p->local;
  // the counts and the layout record: scratch of this call
  const size_t count_bytes = (size_t(rows) * a.groups * 4u + 15u) & ~size_t(15);
  char* tmp = static_cast<char*>(scratch_acquire(count_bytes + sizeof(SetMeta), s));
  int rc = tmp ? BBM_HIP_OK : fail(BBM_HIP_ERR_HIP, "material plan scratch: " + scratch_failure());
  if (!rc)
  {
    a.counts = reinterpret_cast<uint32_t*>(tmp);
    a.meta = reinterpret_cast<SetMeta*>(tmp + count_bytes);
    rc = set_plan_launch(a, s);
    if (!rc)
    {
      // the one host wait of the feature: the segment starts decide the per-row launches of every call on the plan
      err = hipMemcpyAsync(p->seg, a.meta->seg, (rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
      if (err == hipSuccess) err = hipStreamSynchronize(s);
      if (err != hipSuccess)
      {
        (void)hipGetLastError();
        rc = fail(BBM_HIP_ERR_HIP, std::string("material plan failed: ") + hipGetErrorString(err));
      }
    }
    scratch_release(tmp, s);
  }
  for (uint32_t k = 0; !rc && k < rows; ++k)
    if (p->seg[k] > p->seg[k + 1] || (p->seg[k] & 3u) || p->seg[rows] > p->slots || (p->seg[rows] & 3u))
      rc = fail(BBM_HIP_ERR_HIP, "material plan: inconsistent segment offsets");
  if (rc)
  {
    (void)hipFree(p->src);
    return rc;
  }
  *out = p.release();
  return BBM_HIP_OK;
}

int bbm_hip_set_plan_create(const bbm_hip_set* set, const uint32_t* material, size_t n, void* stream,
                            bbm_hip_set_plan** out)
{
  return set_plan_create_common(set, material, n, stream, out, false);
}

int bbm_hip_set_plan_create_compact(const bbm_hip_set* set, const uint32_t* material, size_t n, void* stream,
                                    bbm_hip_set_plan** out)
{
  return set_plan_create_common(set, material, n, stream, out, true);
}

int bbm_hip_set_plan_compact(const bbm_hip_set_plan* plan)
{
  return plan ? int(plan->compact) : fail(BBM_HIP_ERR_INVALID_ARG, "plan is NULL");
}

int bbm_hip_set_plan_destroy(bbm_hip_set_plan* plan)
{
  if (!plan) return BBM_HIP_OK;
  // hipFree waits for the device, so calls already enqueued on the plan finish first
  const hipError_t err = plan->src ? hipFree(plan->src) : hipSuccess;
  delete plan;
  if (err != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("hipFree failed: ") + hipGetErrorString(err));
  return BBM_HIP_OK;
}

size_t bbm_hip_set_plan_lanes(const bbm_hip_set_plan* plan) { return plan ? plan->n : 0u; }

size_t bbm_hip_set_plan_capacity(const bbm_hip_set_plan* plan) { return plan ? plan->seg[plan->set->rows.rows] : 0u; }

int bbm_hip_set_plan_segments(const bbm_hip_set_plan* plan, uint64_t* out, uint32_t count)
{
  if (!plan) return fail(BBM_HIP_ERR_INVALID_ARG, "plan is NULL");
  const uint32_t have = plan->set->rows.rows + 1;
  if (!out || count < have)
    return fail(BBM_HIP_ERR_INVALID_ARG, "segments: room for " + std::to_string(have) + " offsets is needed");
  for (uint32_t k = 0; k < have; ++k) out[k] = plan->seg[k];
  return int(have);
}

const uint32_t* bbm_hip_set_plan_order(const bbm_hip_set_plan* plan) { return plan ? plan->src : nullptr; }

// The three eval + pdf calls on a plan.  lanes: in lane order, `count` lanes; otherwise in plan order, `count` slots.
// tx, ty, tz: all set or all NULL (the call without _tangent).
static int set_eval_pdf_common(bool lanes, const bbm_hip_set_plan* plan, int call_flags,
                               const float* nx, const float* ny, const float* nz,
                               const float* tx, const float* ty, const float* tz,
                               const float* in_x, const float* in_y, const float* in_z,
                               const float* out_x, const float* out_y, const float* out_z,
                               const uint8_t* mask, size_t count, uint32_t component, uint32_t unit,
                               float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  const float* tan[3] = {tx, ty, tz};
  const float* in[9] = {nx, ny, nz, in_x, in_y, in_z, out_x, out_y, out_z};
  float* res[5] = {r, g, b, pdf, cos_in};
  bool world, done;
  const int rc = set_eval_pdf_check(plan, lanes, call_flags, tan, in, mask, count, component, res, world, done);
  if (rc || done) return rc;
  if (!lanes) return set_eval_pdf_rows(*plan, call_flags, world, tan, in, mask, component, unit, res, stream);
  return set_lane_order(set_eval_pdf_rows, *plan, call_flags, world, tan, in, 9, mask, component, unit, res, 5, stream);
}

int bbm_hip_set_eval_pdf(const bbm_hip_set_plan* plan, int call_flags,
                         const float* nx, const float* ny, const float* nz,
                         const float* in_x, const float* in_y, const float* in_z,
                         const float* out_x, const float* out_y, const float* out_z,
                         const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                         float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  return set_eval_pdf_common(true, plan, call_flags, nx, ny, nz, nullptr, nullptr, nullptr, in_x, in_y, in_z, out_x,
                             out_y, out_z, mask, n, component, unit, r, g, b, pdf, cos_in, stream);
}

int bbm_hip_set_eval_pdf_tangent(const bbm_hip_set_plan* plan, int call_flags,
                                 const float* nx, const float* ny, const float* nz,
                                 const float* tx, const float* ty, const float* tz,
                                 const float* in_x, const float* in_y, const float* in_z,
                                 const float* out_x, const float* out_y, const float* out_z,
                                 const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                 float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  return set_eval_pdf_common(true, plan, call_flags, nx, ny, nz, tx, ty, tz, in_x, in_y, in_z, out_x, out_y, out_z,
                             mask, n, component, unit, r, g, b, pdf, cos_in, stream);
}

// The three sample_eval calls on a plan, on the same terms.
static int set_sample_eval_common(bool lanes, const bbm_hip_set_plan* plan, int call_flags,
                                  const float* nx, const float* ny, const float* nz,
                                  const float* tx, const float* ty, const float* tz,
                                  const float* out_x, const float* out_y, const float* out_z,
                                  const float* xi0, const float* xi1,
                                  const uint8_t* mask, size_t count, uint32_t component,
                                  float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                                  float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  const float* tan[3] = {tx, ty, tz};
  const float* in[8] = {nx, ny, nz, out_x, out_y, out_z, xi0, xi1};
  float* res[11] = {dir_x, dir_y, dir_z, pdf, reinterpret_cast<float*>(flag), r, g, b, wr, wg, wb};
  bool world, done;
  const int rc = set_sample_eval_check(plan, lanes, call_flags, tan, in, mask, count, component, res, world, done);
  if (rc || done) return rc;
  if (!lanes) return set_sample_eval_rows(*plan, call_flags, world, tan, in, mask, component, 0u, res, stream);
  return set_lane_order(set_sample_eval_rows, *plan, call_flags, world, tan, in, 8, mask, component, 0u, res, 11, stream);
}

int bbm_hip_set_sample_eval(const bbm_hip_set_plan* plan, int call_flags,
                            const float* nx, const float* ny, const float* nz,
                            const float* out_x, const float* out_y, const float* out_z,
                            const float* xi0, const float* xi1,
                            const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                            float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                            float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  return set_sample_eval_common(true, plan, call_flags, nx, ny, nz, nullptr, nullptr, nullptr, out_x, out_y, out_z, xi0,
                                xi1, mask, n, component, dir_x, dir_y, dir_z, pdf, flag, r, g, b, wr, wg, wb, stream);
}

int bbm_hip_set_sample_eval_tangent(const bbm_hip_set_plan* plan, int call_flags,
                                    const float* nx, const float* ny, const float* nz,
                                    const float* tx, const float* ty, const float* tz,
                                    const float* out_x, const float* out_y, const float* out_z,
                                    const float* xi0, const float* xi1,
                                    const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                                    float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                                    float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  return set_sample_eval_common(true, plan, call_flags, nx, ny, nz, tx, ty, tz, out_x, out_y, out_z, xi0, xi1, mask, n,
                                component, dir_x, dir_y, dir_z, pdf, flag, r, g, b, wr, wg, wb, stream);
}

// ---- material sets in plan order: the permute as a call of its own, and the two calls on streams
// that are already in slot order

// 0: k_set_gather (a stream at a time); 1: k_set_gather_batched.  Process-wide, for bbm_hip_set_plan_gather alone.
static std::atomic<int>& set_gather_shape()
{
  static std::atomic<int> shape{0};
  return shape;
}

int bbm_hip_set_gather_shape(int shape)
{
  if (shape != 0 && shape != 1) return fail(BBM_HIP_ERR_INVALID_ARG, "gather shape: 0 (a stream at a time) or 1 (batched)");
  return set_gather_shape().exchange(shape);
}

// What gather and scatter check, in this order: count and the pointer arrays (which need no plan), the plan, n, and
// for a plan that has slots every entry and the alignment of the slot-order side.  done: nothing to launch.
static int set_move_check(const bbm_hip_set_plan* plan, const void* const* from, void* const* to, int count,
                          const void* const* sorted, size_t n, bool& done)
{
  done = false;
  if (count < 0) return fail(BBM_HIP_ERR_INVALID_ARG, "count is negative");
  if (count > 0 && (!from || !to)) return fail(BBM_HIP_ERR_INVALID_ARG, "from or to is NULL");
  if (!plan) return fail(BBM_HIP_ERR_INVALID_ARG, "plan is NULL");
  if (n != plan->n)
    return fail(BBM_HIP_ERR_INVALID_ARG, "n is " + std::to_string(n) + ", the plan was made for " + std::to_string(plan->n) + " lanes");
  // an empty plan has no slot: its arrays hold nothing and may be NULL
  if ((done = plan->seg[plan->set->rows.rows] == 0)) return BBM_HIP_OK;
  for (int c = 0; c < count; ++c)
    if (!from[c] || !to[c]) return fail(BBM_HIP_ERR_INVALID_ARG, "stream " + std::to_string(c) + ": a NULL pointer");
  for (int c = 0; c < count; ++c)
    if (reinterpret_cast<uintptr_t>(sorted[c]) & 15u)
      return fail(BBM_HIP_ERR_INVALID_ARG, "stream " + std::to_string(c) + ": the array in slot order must be 16-byte aligned");
  return BBM_HIP_OK;
}

int bbm_hip_set_plan_gather(const bbm_hip_set_plan* plan, const void* const* from, void* const* to, int count,
                            const uint8_t* mask_from, uint8_t* mask_to, size_t n, void* stream)
{
  if (mask_from && !mask_to) return fail(BBM_HIP_ERR_INVALID_ARG, "mask_from without mask_to");
  bool done;
  if (const int rc = set_move_check(plan, from, to, count, const_cast<const void* const*>(to), n, done)) return rc;
  if (done || (count == 0 && !mask_to)) return BBM_HIP_OK;
  if (reinterpret_cast<uintptr_t>(mask_to) & 3u) return fail(BBM_HIP_ERR_INVALID_ARG, "mask_to must be 4-byte aligned");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const bool batched = set_gather_shape().load() == 1;
  // kSetMaxIn streams a launch; the mask travels with the first
  for (int first = 0; first == 0 || first < count; first += kSetMaxIn)
  {
    SetMoveArgs m = set_move(*plan);
    for (int c = first; c < count && c < first + kSetMaxIn; ++c) move_in(m, from[c], to[c]);
    if (first == 0) { m.mask_from = mask_from; m.mask_to = mask_to; }
    if (const int rc = batched ? set_gather_launch_batched(m, s) : set_gather_launch(m, s)) return rc;
  }
  return BBM_HIP_OK;
}

int bbm_hip_set_plan_scatter(const bbm_hip_set_plan* plan, const void* const* from, void* const* to, int count,
                             size_t n, void* stream)
{
  bool done;
  if (const int rc = set_move_check(plan, from, to, count, from, n, done)) return rc;
  if (done) return BBM_HIP_OK;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  for (int first = 0; first < count; first += kSetMaxOut)
  {
    SetMoveArgs m = set_move(*plan);
    for (int c = first; c < count && c < first + kSetMaxOut; ++c) move_out(m, const_cast<void*>(from[c]), to[c]);
    if (const int rc = set_scatter_launch(m, s)) return rc;
  }
  return BBM_HIP_OK;
}

int bbm_hip_set_eval_pdf_sorted(const bbm_hip_set_plan* plan, int call_flags,
                                const float* nx, const float* ny, const float* nz,
                                const float* tx, const float* ty, const float* tz,
                                const float* in_x, const float* in_y, const float* in_z,
                                const float* out_x, const float* out_y, const float* out_z,
                                const uint8_t* mask, size_t slots, uint32_t component, uint32_t unit,
                                float* r, float* g, float* b, float* pdf, float* cos_in, void* stream)
{
  return set_eval_pdf_common(false, plan, call_flags, nx, ny, nz, tx, ty, tz, in_x, in_y, in_z, out_x, out_y, out_z,
                             mask, slots, component, unit, r, g, b, pdf, cos_in, stream);
}

int bbm_hip_set_sample_eval_sorted(const bbm_hip_set_plan* plan, int call_flags,
                                   const float* nx, const float* ny, const float* nz,
                                   const float* tx, const float* ty, const float* tz,
                                   const float* out_x, const float* out_y, const float* out_z,
                                   const float* xi0, const float* xi1,
                                   const uint8_t* mask, size_t slots, uint32_t component, uint32_t unit,
                                   float* dir_x, float* dir_y, float* dir_z, float* pdf, uint32_t* flag,
                                   float* r, float* g, float* b, float* wr, float* wg, float* wb, void* stream)
{
  (void)unit;
  return set_sample_eval_common(false, plan, call_flags, nx, ny, nz, tx, ty, tz, out_x, out_y, out_z, xi0, xi1, mask,
                                slots, component, dir_x, dir_y, dir_z, pdf, flag, r, g, b, wr, wg, wb, stream);
}

// ------------------------------------------------------------------------------- doubleRGB (f64.hip)

static int prepare_f64(int model_id, const double* params, int nparams, const f64::F64Launchers*& l,
                       f64::ParamBlockF64& p)
{
  const ModelEntry* e;
  if (const int rc = checked_entry(model_id, nparams, params, true, true, e)) return rc;
  l = &e->run_f64;
  std::memset(&p, 0, sizeof(p));
  for (int i = 0; i < nparams; ++i) p.v[i] = params[i];
  p.v[f64::kMaxParamsF64 - 1] = runtime_id(model_id) ? 1.0 : 0.0;
  return BBM_HIP_OK;
}

int bbm_hip_eval_pdf_f64(int model_id, const double* params, int nparams,
                         const double* in_x, const double* in_y, const double* in_z,
                         const double* out_x, const double* out_y, const double* out_z,
                         const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                         double* r, double* g, double* b, double* pdf, void* stream)
{
  (void)unit;
  const f64::F64Launchers* l;
  f64::EvalArgsF64 a;
  std::memset(&a, 0, sizeof(a));
  int rc = prepare_f64(model_id, params, nparams, l, a.p);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if (!in_x || !in_y || !in_z || !out_x || !out_y || !out_z) return fail(BBM_HIP_ERR_INVALID_ARG, "direction pointer is NULL");
  if (!r || !g || !b || !pdf) return fail(BBM_HIP_ERR_INVALID_ARG, "output pointer is NULL");
  a.ix = in_x; a.iy = in_y; a.iz = in_z; a.ox = out_x; a.oy = out_y; a.oz = out_z;
  a.mask = mask; a.r = r; a.g = g; a.b = b; a.pdf = pdf;
  a.n = n;
  a.component = component & kFlagAll;
  return l->eval_pdf(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_sample_f64(int model_id, const double* params, int nparams,
                       const double* out_x, const double* out_y, const double* out_z,
                       const double* xi0, const double* xi1,
                       const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                       double* dir_x, double* dir_y, double* dir_z, double* pdf, uint32_t* flag, void* stream)
{
  (void)unit;
  const f64::F64Launchers* l;
  f64::SampleArgsF64 a;
  std::memset(&a, 0, sizeof(a));
  int rc = prepare_f64(model_id, params, nparams, l, a.p);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if (!out_x || !out_y || !out_z) return fail(BBM_HIP_ERR_INVALID_ARG, "out direction pointer is NULL");
  if (!xi0 || !xi1) return fail(BBM_HIP_ERR_INVALID_ARG, "xi pointer is NULL");
  if (!dir_x || !dir_y || !dir_z || !pdf || !flag) return fail(BBM_HIP_ERR_INVALID_ARG, "sample output pointer is NULL");
  a.ox = out_x; a.oy = out_y; a.oz = out_z; a.xi0 = xi0; a.xi1 = xi1; a.mask = mask;
  a.dx = dir_x; a.dy = dir_y; a.dz = dir_z; a.pdf = pdf; a.flag = flag;
  a.n = n;
  a.component = component & kFlagAll;
  return l->sample(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_reflectance_f64(int model_id, const double* params, int nparams,
                            const double* out_x, const double* out_y, const double* out_z,
                            const uint8_t* mask, size_t n, uint32_t component, uint32_t unit,
                            double* r, double* g, double* b, void* stream)
{
  (void)unit;
  const f64::F64Launchers* l;
  f64::ReflArgsF64 a;
  std::memset(&a, 0, sizeof(a));
  int rc = prepare_f64(model_id, params, nparams, l, a.p);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if (!out_x || !out_y || !out_z) return fail(BBM_HIP_ERR_INVALID_ARG, "out direction pointer is NULL");
  if (!r || !g || !b) return fail(BBM_HIP_ERR_INVALID_ARG, "reflectance output pointer is NULL");
  a.ox = out_x; a.oy = out_y; a.oz = out_z; a.mask = mask; a.r = r; a.g = g; a.b = b;
  a.n = n;
  a.component = component & kFlagAll;
  return l->reflectance(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_linearizer_size(const bbm_hip_linearizer* lin, uint64_t* size)
{
  LinDesc d;
  int rc = to_desc(lin, d);
  if (rc) return rc;
  if (!size) return fail(BBM_HIP_ERR_INVALID_ARG, "size is NULL");
  *size = lin_size(d);
  return BBM_HIP_OK;
}

int bbm_hip_linearize(const bbm_hip_linearizer* lin, uint64_t begin, size_t n,
                      float* in_x, float* in_y, float* in_z, float* out_x, float* out_y, float* out_z,
                      void* stream)
{
  LinDesc d;
  int rc = to_desc(lin, d);
  if (rc) return rc;
  if (n == 0) return BBM_HIP_OK;
  if (begin + n > lin_size(d)) return fail(BBM_HIP_ERR_INVALID_ARG, "linearizer range out of bounds");
  if (!in_x || !in_y || !in_z || !out_x || !out_y || !out_z)
    return fail(BBM_HIP_ERR_INVALID_ARG, "direction pointer is NULL");
  const unsigned blocks = grid_blocks(n, kBlock, kMaxBlocks);
  hipLaunchKernelGGL(k_linearize, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), d, begin,
                     uint64_t(n), in_x, in_y, in_z, out_x, out_y, out_z);
  return launched();
}

size_t bbm_hip_loss_workspace_size(int nprobes)
{
  // per-block partial sums, then the probes' constructed models (kLossModelBytes each, 256-byte aligned)
  return nprobes > 0 ? size_t(kLossMaxBlocks) * size_t(nprobes) * sizeof(double) + size_t(nprobes) * kLossModelBytes : 0;
}

namespace {
int loss_common(int model_id, const float* probes, int nparams, int nprobes, const float* ref_r, const float* ref_g,
                const float* ref_b, size_t n, int loss_kind, uint32_t component, double* sums, void* workspace,
                size_t workspace_bytes, LossArgs& a, const ModelEntry*& e)
{
  if (const int rc = checked_entry(model_id, nparams, nullptr, false, false, e)) return rc;    // the probes: below
  if (nprobes <= 0) return fail(BBM_HIP_ERR_INVALID_ARG, "nprobes must be positive");
  if (loss_kind < BBM_LOSS_NGAN_L2 || loss_kind > BBM_LOSS_BIERON_LOG) return fail(BBM_HIP_ERR_INVALID_ARG, "unknown loss kind");
  if (!probes || !sums) return fail(BBM_HIP_ERR_INVALID_ARG, "probes / sums pointer is NULL");
  if (n > 0 && (!ref_r || !ref_g || !ref_b)) return fail(BBM_HIP_ERR_INVALID_ARG, "reference pointer is NULL");
  if (!workspace || workspace_bytes < bbm_hip_loss_workspace_size(nprobes))
    return fail(BBM_HIP_ERR_INVALID_ARG, "workspace too small (bbm_hip_loss_workspace_size)");
  std::memset(&a, 0, sizeof(a));
  a.n = n;
  a.ref_r = ref_r; a.ref_g = ref_g; a.ref_b = ref_b;
  a.probes = probes; a.nprobes = nprobes; a.stride = nparams; a.loss_kind = loss_kind;
  a.component = component & kFlagAll;
  a.block_sums = static_cast<double*>(workspace);
  a.models = static_cast<char*>(workspace) + size_t(kLossMaxBlocks) * size_t(nprobes) * sizeof(double);
  a.sums = sums;
  return BBM_HIP_OK;
}
}  // namespace

int bbm_hip_loss(int model_id, const float* probes, int nparams, int nprobes,
                 const bbm_hip_linearizer* lin, uint64_t begin, size_t n,
                 const float* ref_r, const float* ref_g, const float* ref_b,
                 int loss_kind, uint32_t component, uint32_t unit,
                 double* sums, void* workspace, size_t workspace_bytes, void* stream)
{
  (void)unit;
  LinDesc d;
  int rc = to_desc(lin, d);
  if (rc) return rc;
  if (begin + n > lin_size(d)) return fail(BBM_HIP_ERR_INVALID_ARG, "linearizer range out of bounds");
  LossArgs a;
  const ModelEntry* e = nullptr;
  rc = loss_common(model_id, probes, nparams, nprobes, ref_r, ref_g, ref_b, n, loss_kind, component, sums, workspace,
                   workspace_bytes, a, e);
  if (rc) return rc;
  a.lin = d;
  a.begin = begin;
  return e->run.loss(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_loss_pairs(int model_id, const float* probes, int nparams, int nprobes, size_t n,
                       const float* in_x, const float* in_y, const float* in_z,
                       const float* out_x, const float* out_y, const float* out_z,
                       const float* ref_r, const float* ref_g, const float* ref_b,
                       int loss_kind, uint32_t component, uint32_t unit,
                       double* sums, void* workspace, size_t workspace_bytes, void* stream)
{
  (void)unit;
  LossArgs a;
  const ModelEntry* e = nullptr;
  int rc = loss_common(model_id, probes, nparams, nprobes, ref_r, ref_g, ref_b, n, loss_kind, component, sums, workspace,
                       workspace_bytes, a, e);
  if (rc) return rc;
  if (n > 0 && (!in_x || !in_y || !in_z || !out_x || !out_y || !out_z))
    return fail(BBM_HIP_ERR_INVALID_ARG, "direction pointer is NULL");
  a.lin.kind = kLinSpherical;    // unused: the pairs are given
  a.pairs[0] = in_x; a.pairs[1] = in_y; a.pairs[2] = in_z;
  a.pairs[3] = out_x; a.pairs[4] = out_y; a.pairs[5] = out_z;
  return e->run.loss(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_epd_g1_table(float* out, int capacity)
{
  return epd_table_host(out, capacity);
}

int bbm_hip_merl_table(const double* raw, uint32_t theta_h, uint32_t theta_d, uint32_t phi_d, float* table,
                       void* stream)
{
  if (!raw || !table) return fail(BBM_HIP_ERR_INVALID_ARG, "bbm_hip_merl_table: null pointer");
  if (theta_h != uint32_t(kMerlThetaH) || theta_d != uint32_t(kMerlThetaD) || phi_d != uint32_t(kMerlPhiD))
    return fail(BBM_HIP_ERR_INVALID_ARG, "BBM: not a recognized MERL BRDF (dimensions " + std::to_string(theta_h) + " x " +
                                         std::to_string(theta_d) + " x " + std::to_string(phi_d) + ", expected 90 x 90 x 180)");
  return merl_table_launch(raw, table, static_cast<hipStream_t>(stream));
}

size_t bbm_hip_check_workspace_size(const bbm_hip_check_desc* d)
{
  if (!d || d->nslots <= 0) return 0;
  return size_t(d->nslots) * check_blocks(d->n, d->nslots) * kCheckAcc * sizeof(double);
}

int bbm_hip_check(int model_id, const float* params, int nparams, const bbm_hip_check_desc* d,
                  double* acc, uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream)
{
  const CallExactScope mode_scope(model_id);
  const ModelEntry* e;
  if (const int rc = checked_entry(model_id, nparams, params, true, false, e)) return rc;
  if (!d) return fail(BBM_HIP_ERR_INVALID_ARG, "check descriptor is NULL");
  if (d->test < 0 || d->test >= kCheckNumTests) return fail(BBM_HIP_ERR_INVALID_ARG, "unknown check test");
  if (d->nslots <= 0 || d->nslots > 65535) return fail(BBM_HIP_ERR_INVALID_ARG, "nslots must be in [1, 65535]");
  const bool chi2 = d->test == kCheckSamplePdf || d->test == kCheckSampleCount;
  const uint64_t bins = uint64_t(d->theta_bins) * d->phi_bins;
  if (chi2 && (d->theta_bins == 0 || d->phi_bins == 0 || bins > (1u << 20)))
    return fail(BBM_HIP_ERR_INVALID_ARG, "theta_bins / phi_bins must be positive (at most 2^20 bins)");
  if (d->test == kCheckSamplePdf && d->nslots % bins != 0)
    return fail(BBM_HIP_ERR_INVALID_ARG, "SAMPLE_PDF: nslots must be trials x theta_bins x phi_bins");
  const bool needs_dirs = d->test == kCheckReflectance || d->test == kCheckPdfInt || chi2;
  if (needs_dirs && (!d->slot_x || !d->slot_y || !d->slot_z))
    return fail(BBM_HIP_ERR_INVALID_ARG, "this test needs slot directions");
  if (d->test == kCheckSampleCount ? !counts : !acc) return fail(BBM_HIP_ERR_INVALID_ARG, "acc / counts pointer is NULL");
  if (d->test != kCheckSampleCount && (!workspace || workspace_bytes < bbm_hip_check_workspace_size(d)))
    return fail(BBM_HIP_ERR_INVALID_ARG, "workspace too small (bbm_hip_check_workspace_size)");
  CheckArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int k = 0; k < 3; ++k) a.key[k] = check_base_key(d->seed, d->test, k);
  a.begin = d->begin; a.n = d->n; a.nslots = d->nslots;
  a.sx = d->slot_x; a.sy = d->slot_y; a.sz = d->slot_z;
  a.sphere = d->sphere; a.importance = d->importance; a.include_zero = d->include_zero_pdf;
  a.nth = d->theta_bins; a.nph = d->phi_bins;
  a.partial = static_cast<double*>(workspace);
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  for (int i = 0; i < nparams; ++i) a.p.v[i] = params[i];
  a.p.v[kAggregateModeSlot] = runtime_id(model_id) ? 1.0f : 0.0f;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->test == kCheckSampleCount)
  {
    const hipError_t me = hipMemsetAsync(counts, 0, size_t(d->nslots) * bins * sizeof(uint64_t), s);
    if (me != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(me));
  }
  if (d->n == 0 && d->test != kCheckSampleCount)
  {
    const hipError_t me = hipMemsetAsync(acc, 0, size_t(d->nslots) * kCheckAcc * sizeof(double), s);
    return me == hipSuccess ? BBM_HIP_OK : fail(BBM_HIP_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(me));
  }
  if (d->n == 0) return BBM_HIP_OK;
  return e->run.check(d->test, a, acc, s);
}

// ------------------------------------------------------------------------------- image tools (image.hpp)

namespace {
// bbm::normalize on the host, in float: t * (1 / sqrt(|t|^2)) (backbone horizontal.h:105-109); false for a zero or
// non-finite vector
bool normalize_host(const float* v, float* o)
{
  if (!v) return false;
  const float sq = ((0.0f + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2];
  if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2]) || !std::isfinite(sq) || !(sq > 0.0f)) return false;
  const float r = 1.0f / std::sqrt(sq);
  for (int k = 0; k < 3; ++k) o[k] = v[k] * r;
  return std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]);
}

int image_size(uint32_t width, uint32_t height)
{
  if (width == 0 || height == 0) return fail(BBM_HIP_ERR_INVALID_ARG, "image width and height must be positive");
  if (uint64_t(width) * height > kImageMaxPixels) return fail(BBM_HIP_ERR_INVALID_ARG, "image has more than 2^31 pixels");
  return BBM_HIP_OK;
}

// renderSphere.cpp:114, :129: light = normalize(light); render(..., -normalize(light), ...)
int render_light(const float* light, v3& dir)
{
  float l1[3], l2[3];
  if (!normalize_host(light, l1) || !normalize_host(l1, l2))
    return fail(BBM_HIP_ERR_INVALID_ARG, "light must be a finite non-zero vector");
  dir.x = -l2[0]; dir.y = -l2[1]; dir.z = -l2[2];
  return BBM_HIP_OK;
}

// plotBsdf.cpp:113-142 and the draws: kind, samples, view = normalize(view), xi / key
int plot_args(int kind, uint32_t width, uint32_t height, const float* view, uint64_t samples, float scale,
              const float* xi0, const float* xi1, uint64_t seed, ImageArgs& a)
{
  if (kind != kPlotEval && kind != kPlotPdf && kind != kPlotSample) return fail(BBM_HIP_ERR_INVALID_ARG, "unknown plot kind");
  if (const int rc = image_size(width, height)) return rc;
  if (samples == 0) return fail(BBM_HIP_ERR_INVALID_ARG, "samples must be positive");
  if (samples > (uint64_t(1) << 40) / (uint64_t(width) * height) + 1)
    return fail(BBM_HIP_ERR_INVALID_ARG, "width x height x samples exceeds 2^40 draws");
  float v[3];
  if (!normalize_host(view, v)) return fail(BBM_HIP_ERR_INVALID_ARG, "view must be a finite non-zero vector");
  if ((xi0 == nullptr) != (xi1 == nullptr)) return fail(BBM_HIP_ERR_INVALID_ARG, "xi0 and xi1 must both be given or both be NULL");
  a.op = kind;
  a.width = width; a.height = height; a.samples = samples;
  a.dir.x = v[0]; a.dir.y = v[1]; a.dir.z = v[2];
  a.scale = scale;
  a.key = plot_key(seed);
  a.xi0 = xi0; a.xi1 = xi1;
  return BBM_HIP_OK;
}
}  // namespace

int bbm_hip_render_sphere(int model_id, const float* params, int nparams, uint32_t width, uint32_t height,
                          const float* light, float* image, float* in_x, float* in_y, float* in_z,
                          float* out_x, float* out_y, float* out_z, uint8_t* mask, void* stream)
{
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  const ModelEntry* e;
  int rc = prepare(model_id, params, nparams, 0, tmp, e);
  if (rc) return rc;
  if ((rc = image_size(width, height))) return rc;
  if (!image) return fail(BBM_HIP_ERR_INVALID_ARG, "image pointer is NULL");
  if ((in_x || in_y || in_z) && !(in_x && in_y && in_z)) return fail(BBM_HIP_ERR_INVALID_ARG, "in direction pointer is NULL");
  if ((out_x || out_y || out_z) && !(out_x && out_y && out_z)) return fail(BBM_HIP_ERR_INVALID_ARG, "out direction pointer is NULL");
  ImageArgs a;
  std::memset(&a, 0, sizeof(a));
  if ((rc = render_light(light, a.dir))) return rc;
  a.op = kImageRender;
  a.width = width; a.height = height; a.samples = 1; a.scale = 1.0f;
  a.img = image;
  a.ix = in_x; a.iy = in_y; a.iz = in_z; a.ox = out_x; a.oy = out_y; a.oz = out_z; a.mask = mask;
  a.p = tmp.p;
  return e->run.image(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_render_sphere_dirs(uint32_t width, uint32_t height, const float* light, float* in_x, float* in_y, float* in_z,
                               float* out_x, float* out_y, float* out_z, uint8_t* mask, void* stream)
{
  int rc = image_size(width, height);
  if (rc) return rc;
  if (!in_x || !in_y || !in_z || !out_x || !out_y || !out_z || !mask)
    return fail(BBM_HIP_ERR_INVALID_ARG, "direction / mask pointer is NULL");
  ImageArgs a;
  std::memset(&a, 0, sizeof(a));
  if ((rc = render_light(light, a.dir))) return rc;
  a.op = kImageRender;
  a.width = width; a.height = height; a.samples = 1;
  a.ix = in_x; a.iy = in_y; a.iz = in_z; a.ox = out_x; a.oy = out_y; a.oz = out_z; a.mask = mask;
  return sphere_dirs_launch(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_render_shade(size_t npixels, const float* r, const float* g, const float* b, const float* in_z,
                         const uint8_t* mask, float* image, void* stream)
{
  if (npixels == 0 || uint64_t(npixels) > kImageMaxPixels) return fail(BBM_HIP_ERR_INVALID_ARG, "pixel count must be in [1, 2^31]");
  if (!r || !g || !b || !in_z || !mask) return fail(BBM_HIP_ERR_INVALID_ARG, "input pointer is NULL");
  if (!image) return fail(BBM_HIP_ERR_INVALID_ARG, "image pointer is NULL");
  return render_shade_launch(npixels, r, g, b, in_z, mask, image, static_cast<hipStream_t>(stream));
}

int bbm_hip_plot(int model_id, const float* params, int nparams, int kind, uint32_t width, uint32_t height,
                 const float* view, uint64_t samples, float scale, int mask_zero, const float* xi0, const float* xi1,
                 uint64_t seed, float* image, uint64_t* counts, void* stream)
{
  const CallExactScope mode_scope(model_id);
  EvalArgs tmp;
  const ModelEntry* e;
  int rc = prepare(model_id, params, nparams, 0, tmp, e);
  if (rc) return rc;
  ImageArgs a;
  std::memset(&a, 0, sizeof(a));
  if ((rc = plot_args(kind, width, height, view, samples, scale, xi0, xi1, seed, a))) return rc;
  if (!image) return fail(BBM_HIP_ERR_INVALID_ARG, "image pointer is NULL");
  if (kind == kPlotSample && !counts) return fail(BBM_HIP_ERR_INVALID_ARG, "counts pointer is NULL");
  a.mask_zero = mask_zero;
  a.img = image;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.p = tmp.p;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (kind == kPlotSample)
  {
    const hipError_t me = hipMemsetAsync(counts, 0, size_t(width) * height * sizeof(uint64_t), s);
    if (me != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(me));
  }
  return e->run.image(a, s);
}

int bbm_hip_plot_dirs(uint32_t width, uint32_t height, uint64_t samples, const float* xi0, const float* xi1, uint64_t seed,
                      float* x, float* y, float* z, void* stream)
{
  const float view[3] = {0.0f, 0.0f, 1.0f};
  ImageArgs a;
  std::memset(&a, 0, sizeof(a));
  int rc = plot_args(kPlotEval, width, height, view, samples, 1.0f, xi0, xi1, seed, a);
  if (rc) return rc;
  if (!x || !y || !z) return fail(BBM_HIP_ERR_INVALID_ARG, "direction pointer is NULL");
  a.ix = x; a.iy = y; a.iz = z;
  return plot_dirs_launch(a, static_cast<hipStream_t>(stream));
}

int bbm_hip_plot_accumulate(int kind, uint32_t width, uint32_t height, uint64_t samples, float scale, const float* xi0,
                            const float* xi1, uint64_t seed, const float* r, const float* g, const float* b, float* image,
                            void* stream)
{
  const float view[3] = {0.0f, 0.0f, 1.0f};
  ImageArgs a;
  std::memset(&a, 0, sizeof(a));
  if (kind != kPlotEval && kind != kPlotPdf) return fail(BBM_HIP_ERR_INVALID_ARG, "unknown plot kind");
  int rc = plot_args(kind, width, height, view, samples, scale, xi0, xi1, seed, a);
  if (rc) return rc;
  if (!r || (kind == kPlotEval && (!g || !b))) return fail(BBM_HIP_ERR_INVALID_ARG, "input pointer is NULL");
  if (!image) return fail(BBM_HIP_ERR_INVALID_ARG, "image pointer is NULL");
  a.img = image;
  return plot_accumulate_launch(a, r, g, b, static_cast<hipStream_t>(stream));
}

int bbm_hip_plot_bin(uint32_t width, uint32_t height, size_t n, const float* dir_x, const float* dir_y, const float* dir_z,
                     const float* pdf, int mask_zero, uint64_t* counts, void* stream)
{
  int rc = image_size(width, height);
  if (rc) return rc;
  if (!counts) return fail(BBM_HIP_ERR_INVALID_ARG, "counts pointer is NULL");
  if (n > 0 && (!dir_x || !dir_y || !dir_z || !pdf)) return fail(BBM_HIP_ERR_INVALID_ARG, "direction / pdf pointer is NULL");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t me = hipMemsetAsync(counts, 0, size_t(width) * height * sizeof(uint64_t), s);
  if (me != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(me));
  if (n == 0) return BBM_HIP_OK;
  return plot_bin_launch(width, height, n, dir_x, dir_y, dir_z, pdf, mask_zero, reinterpret_cast<unsigned long long*>(counts), s);
}

int bbm_hip_plot_counts_image(const uint64_t* counts, uint32_t width, uint32_t height, uint64_t samples, float scale,
                              float* image, void* stream)
{
  int rc = image_size(width, height);
  if (rc) return rc;
  if (samples == 0) return fail(BBM_HIP_ERR_INVALID_ARG, "samples must be positive");
  if (!counts) return fail(BBM_HIP_ERR_INVALID_ARG, "counts pointer is NULL");
  if (!image) return fail(BBM_HIP_ERR_INVALID_ARG, "image pointer is NULL");
  return count_image_launch(reinterpret_cast<const unsigned long long*>(counts), width, height, samples, scale, image,
                            static_cast<hipStream_t>(stream));
}

int bbm_hip_plot_draws(uint64_t seed, uint64_t offset, size_t n, float* xi0, float* xi1, void* stream)
{
  if (n == 0) return BBM_HIP_OK;
  if (!xi0 || !xi1) return fail(BBM_HIP_ERR_INVALID_ARG, "xi pointer is NULL");
  return plot_draws_launch(seed, offset, n, xi0, xi1, static_cast<hipStream_t>(stream));
}

int bbm_hip_check_draws(int test, uint64_t seed, int slot, int draw, uint64_t offset, size_t n,
                        float* xi0, float* xi1, void* stream)
{
  if (n == 0) return BBM_HIP_OK;
  if (!xi0 || !xi1) return fail(BBM_HIP_ERR_INVALID_ARG, "xi pointer is NULL");
  if (test < 0 || test >= kCheckNumTests || draw < 0 || draw > 2 || slot < 0)
    return fail(BBM_HIP_ERR_INVALID_ARG, "test / draw / slot out of range");
  const unsigned blocks = grid_blocks(n, kBlock, kMaxBlocks);
  hipLaunchKernelGGL(k_draws, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     check_key(check_base_key(seed, test, draw), slot), offset, uint64_t(n), xi0, xi1);
  return launched();
}

int bbm_hip_check_trials(int test, uint64_t seed, int ntrials, int sphere, float* x, float* y, float* z, void* stream)
{
  if (ntrials <= 0) return ntrials == 0 ? BBM_HIP_OK : fail(BBM_HIP_ERR_INVALID_ARG, "ntrials < 0");
  if (!x || !y || !z) return fail(BBM_HIP_ERR_INVALID_ARG, "direction pointer is NULL");
  if (test < 0 || test >= kCheckNumTests) return fail(BBM_HIP_ERR_INVALID_ARG, "unknown check test");
  // the trial direction is its own stream (draw index 3), sample 0
  hipLaunchKernelGGL(k_trials, dim3(unsigned((ntrials + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), check_base_key(seed, test, 3), ntrials, sphere, x, y, z);
  return launched();
}

int bbm_hip_sphere_dirs(const float* xi0, const float* xi1, size_t n, int hemisphere, float* x, float* y, float* z,
                        void* stream)
{
  if (n == 0) return BBM_HIP_OK;
  if (!xi0 || !xi1 || !x || !y || !z) return fail(BBM_HIP_ERR_INVALID_ARG, "pointer is NULL");
  const unsigned blocks = grid_blocks(n, kBlock, kMaxBlocks);
  hipLaunchKernelGGL(k_sphere_dirs, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), xi0, xi1,
                     uint64_t(n), hemisphere, x, y, z);
  return launched();
}

int bbm_hip_libm_eval(int func, const float* a, const float* b, float* out, size_t n, void* stream)
{
  if (n == 0) return BBM_HIP_OK;
  if (func < BBM_HIP_LIBM_EXPF || func > BBM_HIP_LIBM_THETA)
    return fail(BBM_HIP_ERR_INVALID_ARG, "unknown libm function");
  if (!a || !out || ((func == BBM_HIP_LIBM_POWF || func == BBM_HIP_LIBM_ONE_PLUS_SQRT || func == BBM_HIP_LIBM_ATAN2F || func == BBM_HIP_LIBM_THETA) && !b)) return fail(BBM_HIP_ERR_INVALID_ARG, "pointer is NULL");
  const unsigned blocks = grid_blocks(n, kBlock, kMaxBlocks);
  hipLaunchKernelGGL(k_libm, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), func, a, b, out,
                     uint64_t(n));
  return launched();
}

int bbm_hip_fill_directions(uint64_t seed, uint32_t stream_id, uint64_t offset, size_t n, int mode,
                            float* x, float* y, float* z, void* stream)
{
  if (n == 0) return BBM_HIP_OK;
  if (!x || !y || !z) return fail(BBM_HIP_ERR_INVALID_ARG, "direction pointer is NULL");
  if (mode != 0 && mode != 1) return fail(BBM_HIP_ERR_INVALID_ARG, "mode must be 0 (hemisphere) or 1 (sphere)");
  const unsigned blocks = grid_blocks(n, kBlock, kMaxBlocks);
  const uint64_t key = mix64(seed) ^ (0xd1b54a32d192ed03ull * (uint64_t(stream_id) + 1));
  hipLaunchKernelGGL(k_fill_dirs, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), key,
                     offset, uint64_t(n), mode, x, y, z);
  return launched();
}

}  // extern "C"
