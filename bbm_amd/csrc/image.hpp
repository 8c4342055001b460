// bbm_amd/csrc/image.hpp -- bin/renderSphere and bin/plotBsdf as image-space kernels.
//
// Both reference tools evaluate a BSDF once per pixel (and per sample) at directions made on the fly and write an
// image; nothing is read from HBM, so the kernels are compute-bound.  floatRGB only, as the tools are
// (BBM_IMPORT_CONFIG(floatRGB)).  Images are (3, H, W) planes, row y = 0 first.
//
//   render (renderSphere.cpp:17-58): the sphere's normal map (:17-33), transpose(toGlobalShadingFrame(n))
//     (core/shading_frame.h:26-58, Duff et al.'s basis), in = sf * lightdir, out = sf * (0, 0, 1),
//     pixel = eval(in, out) * |z(in)| where |n|^2 > eps, 0 elsewhere.  One thread per pixel.
//   plot eval / pdf (plotBsdf.cpp:15-62): per pixel the `samples` loop runs inside the thread, in order, so the
//     float sum is the reference's.  Draw (pixel * samples + s) gives (u_phi, u_theta).
//   plot sample (plotBsdf.cpp:65-86): one thread per draw increments its bin's integer count (atomics: exact and
//     order-independent); the reference adds the same double constant to a float bin every time, so the bin's final
//     float depends on its count alone and count_image_launch replays that many additions.
//
// Random numbers: uniform2 (check.hpp) on plot_key(seed), a stream no check_base_key stream shares, indexed by the
// global draw index -- or the caller's own uniforms, xi0[g] / xi1[g].
//
// The staged path (image.hip) makes the same directions and weights with the same device functions below, for
// models without a fused kernel (composed aggregates, runtime trees): directions -> the tree's eval / pdf / sample
// entry points -> shade / accumulate / bin.  Same functions, same order: the same image bit for bit.
#pragma once
#include "math.hpp"
#include "frame.hpp"
#include "fit.hpp"    // sph_to_vec, phi_of, theta_of, cossin_cr
#include "check.hpp"   // uniform2, check_base_key, check_key

namespace bbmhip {

enum : int { kPlotEval = 0, kPlotPdf = 1, kPlotSample = 2, kImageRender = 3 };
constexpr uint64_t kImageMaxPixels = uint64_t(1) << 31;
constexpr int kImageMaxBlocks = 1 << 16;     // grid cap of the per-draw kernels (grid-stride)

struct ImageArgs
{
  int op;                       // kPlotEval / kPlotPdf / kPlotSample / kImageRender
  uint32_t width, height;
  uint64_t samples;
  v3 dir;                       // render: -normalize(normalize(light)); plot: normalize(view)
  float scale;
  int mask_zero;
  uint64_t key;                 // plot_key(seed)
  const float* xi0; const float* xi1;      // caller's uniforms per draw, or nullptr
  float* img;                   // (3, H, W)
  float* ix; float* iy; float* iz;         // render: in per pixel, or nullptr
  float* ox; float* oy; float* oz;         // render: out per pixel, or nullptr
  uint8_t* mask;                // render: shaded mask per pixel, or nullptr
  unsigned long long* counts;   // plot sample: [H * W], zeroed by the caller
  ParamBlock p;
};

// the plot tools' draw stream: test index 0x100 is beyond every checkBsdf test (check_base_key), slot 0
__host__ __device__ __forceinline__ uint64_t plot_key(uint64_t seed) { return check_key(check_base_key(seed, 0x100, 0), 0); }

__device__ __forceinline__ void plot_draw(const ImageArgs& a, uint64_t g, float& u0, float& u1)
{
  if (a.xi0 != nullptr) { u0 = a.xi0[g]; u1 = a.xi1[g]; }
  else uniform2(a.key, g, u0, u1);
}

// renderSphere.cpp:17-33 and :46-52: the pixel's normal, shading frame and local directions.  Returns whether the
// pixel is shaded (|n|^2 > eps); in / out are 0 where it is not.
__device__ __forceinline__ bool sphere_pixel(uint32_t x, uint32_t y, uint32_t w, uint32_t h, v3 light, v3& in, v3& out)
{
  const float radius = float(w < h ? w : h) / 2.0f;             // std::min(width, height) / 2.0f
  const float cx = float(w / 2u), cy = float(h / 2u);           // Vec3d center(width / 2, height / 2, 0): integer division
  v3 n = mk3(div_nr(cx - float(x), radius), div_nr(cy - float(y), radius), 0.0f);
  const float len = dot3(n, n);
  if (len < 1.0f) n.z = sqrt_nr(1.0f - len);
  else n = mk3(0.0f, 0.0f, 0.0f);
  in = out = mk3(0.0f, 0.0f, 0.0f);
  // transpose(toGlobalShadingFrame(n)) * v (frame.hpp)
  const Frame f = shading_frame(n);
  if (!f.live) return false;
  in = f.to_local(light);
  out = f.to_local(mk3(0.0f, 0.0f, 1.0f));
  return true;
}

// plotBsdf.cpp:26-28: the light direction of pixel (x, y) for the draw (u_phi, u_theta); theta is returned for pdf's weight
__device__ __forceinline__ v3 plot_light(uint32_t x, uint32_t y, uint32_t w, uint32_t h, float u_phi, float u_theta, float& theta)
{
  const float phi = div_nr(kPi2F * (float(x) + u_phi), float(w));
  theta = div_nr(kPiF * (float(y) + u_theta), float(h));
  return sph_to_vec(phi, theta);
}

// plotBsdf.cpp:30: one sample's term, eval * cosTheta(light) / samples
__device__ __forceinline__ float plot_eval_term(float f, v3 light, float fsamples) { return div_nr(f * light.z, fsamples); }

// plotBsdf.cpp:53: Pi2(2) |sinTheta| / (width * height)
__device__ __forceinline__ float plot_pdf_weight(float theta, float fpixels)
{
  float st, ct;
  cossin_cr(theta, ct, st);
  constexpr float kPiSq2 = (2.0f * kPiF) * kPiF;      // Constants::Pi2(2) = scale * Pi() * Pi() in float
  return div_nr(kPiSq2 * fabsf(st), fpixels);
}

// plotBsdf.cpp:74-77: the bin of a sampled direction, clamped to the last column / row
__device__ __forceinline__ uint32_t plot_bin(v3 dir, uint32_t w, uint32_t h)
{
  const float px = fminf(phi_of(dir) / kPi2F * float(w), float(w - 1u));
  const float py = fminf(theta_of(dir) / kPiF * float(h), float(h - 1u));
  return uint32_t(py) * w + uint32_t(px);
}

// minimum waves per SIMD of the image kernels: the checkBsdf kernels' choice (check.hpp, models.hpp) -- the same
// model code (eval, pdf and the samplers) behind a few dozen instructions of geometry
template<class Model> struct image_waves { static constexpr int value = check_waves<Model>::value; };

template<class Model, bool EXACT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(image_waves<Model>::value, 8))) void k_render_sphere(ImageArgs a)
{
  math_tables_init();
  const Model m(a.p.v);
  const uint64_t npix = uint64_t(a.width) * a.height;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= npix) return;
  const uint32_t y = uint32_t(i / a.width), x = uint32_t(i % a.width);
  v3 in, out;
  const bool shaded = sphere_pixel(x, y, a.width, a.height, a.dir, in, out);
  float f[3] = {0.0f, 0.0f, 0.0f}, unused;
  if (shaded)
  {
    model_eval_pdf<kModeEval, EXACT>(m, in, out, kFlagAll, f, unused);
    const float c = fabsf(in.z);
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = f[k] * c;
  }
  a.img[i] = f[0]; a.img[npix + i] = f[1]; a.img[2 * npix + i] = f[2];
  if (a.ix != nullptr) { a.ix[i] = in.x; a.iy[i] = in.y; a.iz[i] = in.z; }
  if (a.ox != nullptr) { a.ox[i] = out.x; a.oy[i] = out.y; a.oz[i] = out.z; }
  if (a.mask != nullptr) a.mask[i] = shaded ? 1 : 0;
}

template<class Model, int KIND, bool EXACT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(image_waves<Model>::value, 8))) void k_plot(ImageArgs a)
{
  math_tables_init();
  const Model m(a.p.v);
  const uint64_t npix = uint64_t(a.width) * a.height;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= npix) return;
  const uint32_t y = uint32_t(i / a.width), x = uint32_t(i % a.width);
  const float fsamples = float(a.samples), fpixels = float(npix);
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (uint64_t s = 0; s < a.samples; ++s)
  {
    float u0, u1, theta, f[3], p;
    plot_draw(a, i * a.samples + s, u0, u1);
    const v3 light = plot_light(x, y, a.width, a.height, u0, u1, theta);
    if constexpr (KIND == kPlotEval)
    {
      model_eval_pdf<kModeEval, EXACT>(m, light, a.dir, kFlagAll, f, p);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] += plot_eval_term(f[k], light, fsamples);
    }
    else
    {
      model_eval_pdf<kModePdf, EXACT>(m, light, a.dir, kFlagAll, f, p);
      const float t = p * plot_pdf_weight(theta, fpixels);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] += t;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    if (KIND == kPlotPdf) acc[k] = div_nr(acc[k], fsamples);
    a.img[uint64_t(k) * npix + i] = acc[k] * a.scale;
  }
}

template<class Model>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(image_waves<Model>::value, 8))) void k_plot_sample(ImageArgs a)
{
  math_tables_init();
  const Model m(a.p.v);
  const uint64_t npix = uint64_t(a.width) * a.height;
  const uint64_t n = npix * a.samples;
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x; g < n; g += stride)
  {
    float u0, u1, pdf;
    v3 dir; uint32_t flag;
    plot_draw(a, g, u0, u1);
    m.sample(a.dir, u0, u1, kFlagAll, dir, pdf, flag);
    if (!a.mask_zero || pdf > kEpsF)
    {
      const uint32_t idx = plot_bin(dir, a.width, a.height);
      if (idx < npix) atomicAdd(a.counts + idx, 1ull);
    }
  }
}

// staged path and the count replay (image.hip)
int count_image_launch(const unsigned long long* counts, uint32_t width, uint32_t height, uint64_t samples, float scale,
                       float* img, hipStream_t s);
int plot_draws_launch(uint64_t seed, uint64_t offset, uint64_t n, float* xi0, float* xi1, hipStream_t s);
int sphere_dirs_launch(const ImageArgs& a, hipStream_t s);                  // a.ix .. a.oz, a.mask
int render_shade_launch(uint64_t npix, const float* r, const float* g, const float* b, const float* iz, const uint8_t* mask,
                        float* img, hipStream_t s);
int plot_dirs_launch(const ImageArgs& a, hipStream_t s);                    // a.ix / iy / iz: one light direction per draw
int plot_accumulate_launch(const ImageArgs& a, const float* r, const float* g, const float* b, hipStream_t s);
int plot_bin_launch(uint32_t w, uint32_t h, uint64_t n, const float* dx, const float* dy, const float* dz, const float* pdf,
                    int mask_zero, unsigned long long* counts, hipStream_t s);

template<class K, int KIND, bool EXACT>
void launch_plot_kernel(dim3 grid, const ImageArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL((k_plot<K, KIND, EXACT>), grid, dim3(kBlock), 0, s, a);
}

template<class Model>
int launch_image(const ImageArgs& a0, hipStream_t s)
{
  if (const int rc = host_prepare<Model>::run(s)) return rc;
  if (const int rc = host_validate<Model>::run(a0.p)) return rc;
  ImageArgs a = a0;
  void* scratch = nullptr;
  if (const int rc = host_params<Model>::run(a.p, kFlagAll, s, &scratch)) return rc;
  struct Release { void* p; hipStream_t s; ~Release() { host_params<Model>::done(p, s); } } release{scratch, s};
  const uint64_t npix = uint64_t(a.width) * a.height;
  const dim3 grid(unsigned((npix + kBlock - 1) / kBlock));
  bool exact = false;
  if constexpr (model_has_exact<Model>()) exact = exact_on();
  switch (a.op)
  {
    case kImageRender:
      if constexpr (model_has_exact<Model>())
        if (exact) { hipLaunchKernelGGL((k_render_sphere<Model, true>), grid, dim3(kBlock), 0, s, a); break; }
      hipLaunchKernelGGL((k_render_sphere<Model, false>), grid, dim3(kBlock), 0, s, a);
      break;
    case kPlotEval:
      if constexpr (model_has_exact<Model>())
        if (exact) { launch_plot_kernel<Model, kPlotEval, true>(grid, a, s); break; }
      launch_plot_kernel<Model, kPlotEval, false>(grid, a, s);
      break;
    case kPlotPdf:
      if constexpr (model_has_exact<Model>())
        if (exact) { launch_plot_kernel<Model, kPlotPdf, true>(grid, a, s); break; }
      launch_plot_kernel<Model, kPlotPdf, false>(grid, a, s);
      break;
    case kPlotSample:
    {
      uint64_t b = (npix * a.samples + kBlock - 1) / kBlock;
      if (b > uint64_t(kImageMaxBlocks)) b = kImageMaxBlocks;
      bool launched = false;
      if constexpr (has_exact_sample<Model>())       // exact mode: the sampler's twin with glibc's erff / logf (math.hpp)
        if (exact_on())
        {
          hipLaunchKernelGGL((k_plot_sample<exact_sample_t<Model>>), dim3(unsigned(b)), dim3(kBlock), 0, s, a);
          launched = true;
        }
      if (!launched) hipLaunchKernelGGL((k_plot_sample<Model>), dim3(unsigned(b)), dim3(kBlock), 0, s, a);
      if (const int rc = count_image_launch(a.counts, a.width, a.height, a.samples, a.scale, a.img, s)) return rc;
      break;
    }
    default: return fail(BBM_HIP_ERR_INVALID_ARG, "unknown image operation");
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string("kernel launch failed: ") + hipGetErrorString(e));
  return BBM_HIP_OK;
}

}  // namespace bbmhip
