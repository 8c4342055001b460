// bbm_amd/csrc/image.hip -- the model-independent kernels of the image tools (image.hpp): the count replay of
// plot `sample`, the draw generator, and the staged path for models without a fused image kernel (composed
// aggregates, runtime trees): directions -> the tree's own eval / pdf / sample entry points -> shade / accumulate /
// bin.  Directions, weights and summation order come from image.hpp's device functions, as in the fused kernels.
#include "kernels.hpp"

namespace bbmhip {

namespace {

// plotBsdf.cpp:80: result(x, y) += 1.0 / (float)(width * height * samples) -- array<float, 3> += double is
// r = float(double(r) + v) per channel (backbone/array.h:87).  The addend never changes, so the bin holds what `count`
// such additions from 0 leave; the loop stops early once an addition no longer moves the float (it never will again).
__global__ __launch_bounds__(kBlock) void k_count_image(const unsigned long long* counts, uint64_t npix, double addend,
                                                        float scale, float* img)
{
  math_tables_init();
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= npix) return;
  const unsigned long long c = counts[i];
  float v = 0.0f;
  for (unsigned long long k = 0; k < c; ++k)
  {
    const float nv = float(double(v) + addend);
    if (nv == v) break;
    v = nv;
  }
  const float r = v * scale;
  img[i] = r; img[npix + i] = r; img[2 * npix + i] = r;
}

__global__ __launch_bounds__(kBlock) void k_plot_draws(uint64_t key, uint64_t offset, uint64_t n, float* u0, float* u1)
{
  math_tables_init();
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) uniform2(key, offset + i, u0[i], u1[i]);
}

__global__ __launch_bounds__(kBlock) void k_sphere_pixel_dirs(ImageArgs a)
{
  math_tables_init();
  const uint64_t npix = uint64_t(a.width) * a.height;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= npix) return;
  v3 in, out;
  const bool shaded = sphere_pixel(uint32_t(i % a.width), uint32_t(i / a.width), a.width, a.height, a.dir, in, out);
  a.ix[i] = in.x; a.iy[i] = in.y; a.iz[i] = in.z;
  a.ox[i] = out.x; a.oy[i] = out.y; a.oz[i] = out.z;
  a.mask[i] = shaded ? 1 : 0;
}

// pixel = eval(in, out) * |z(in)| where shaded, 0 elsewhere (renderSphere.cpp:41, :53)
__global__ __launch_bounds__(kBlock) void k_render_shade(uint64_t npix, const float* r, const float* g, const float* b,
                                                         const float* iz, const uint8_t* mask, float* img)
{
  math_tables_init();
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= npix) return;
  const bool shaded = mask[i] != 0;
  const float c = fabsf(iz[i]);
  img[i] = shaded ? r[i] * c : 0.0f;
  img[npix + i] = shaded ? g[i] * c : 0.0f;
  img[2 * npix + i] = shaded ? b[i] * c : 0.0f;
}

// light direction of every draw g = pixel * samples + s (ix / iy / iz: [H * W * samples])
__global__ __launch_bounds__(kBlock) void k_plot_light_dirs(ImageArgs a)
{
  math_tables_init();
  const uint64_t n = uint64_t(a.width) * a.height * a.samples;
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x; g < n; g += stride)
  {
    const uint64_t i = g / a.samples;
    float u0, u1, theta;
    plot_draw(a, g, u0, u1);
    const v3 l = plot_light(uint32_t(i % a.width), uint32_t(i / a.width), a.width, a.height, u0, u1, theta);
    a.ix[g] = l.x; a.iy[g] = l.y; a.iz[g] = l.z;
  }
}

// per pixel, in sample order: eval's terms f * cosTheta / samples, or pdf's p * weight and one division at the end
// (the fused k_plot's loop over materialised values; r / g / b: [H * W * samples], pdf kind reads r only)
template<int KIND>
__global__ __launch_bounds__(kBlock) void k_plot_accumulate(ImageArgs a, const float* r, const float* g, const float* b)
{
  math_tables_init();
  const uint64_t npix = uint64_t(a.width) * a.height;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= npix) return;
  const uint32_t y = uint32_t(i / a.width), x = uint32_t(i % a.width);
  const float fsamples = float(a.samples), fpixels = float(npix);
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (uint64_t s = 0; s < a.samples; ++s)
  {
    const uint64_t d = i * a.samples + s;
    float u0, u1, theta;
    plot_draw(a, d, u0, u1);
    const v3 light = plot_light(x, y, a.width, a.height, u0, u1, theta);
    if constexpr (KIND == kPlotEval)
    {
      acc[0] += plot_eval_term(r[d], light, fsamples);
      acc[1] += plot_eval_term(g[d], light, fsamples);
      acc[2] += plot_eval_term(b[d], light, fsamples);
    }
    else
    {
      const float t = r[d] * plot_pdf_weight(theta, fpixels);
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

__global__ __launch_bounds__(kBlock) void k_plot_bin(uint32_t w, uint32_t h, uint64_t n, const float* dx, const float* dy,
                                                     const float* dz, const float* pdf, int mask_zero,
                                                     unsigned long long* counts)
{
  math_tables_init();
  const uint64_t npix = uint64_t(w) * h;
  const uint64_t stride = uint64_t(gridDim.x) * kBlock;
  for (uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x; g < n; g += stride)
    if (!mask_zero || pdf[g] > kEpsF)
    {
      const uint32_t idx = plot_bin(mk3(dx[g], dy[g], dz[g]), w, h);
      if (idx < npix) atomicAdd(counts + idx, 1ull);
    }
}

unsigned pixel_blocks(uint64_t npix) { return unsigned((npix + kBlock - 1) / kBlock); }
unsigned draw_blocks(uint64_t n)
{
  uint64_t b = (n + kBlock - 1) / kBlock;
  if (b > uint64_t(kImageMaxBlocks)) b = kImageMaxBlocks;
  return unsigned(b < 1 ? 1 : b);
}

}  // namespace

int count_image_launch(const unsigned long long* counts, uint32_t width, uint32_t height, uint64_t samples, float scale,
                       float* img, hipStream_t s)
{
  const uint64_t npix = uint64_t(width) * height;
  const double addend = 1.0 / double(float(npix * samples));      // 1.0 / (float)(width * height * samples)
  hipLaunchKernelGGL(k_count_image, dim3(pixel_blocks(npix)), dim3(kBlock), 0, s, counts, npix, addend, scale, img);
  return launched("count replay: kernel launch failed");
}

int plot_draws_launch(uint64_t seed, uint64_t offset, uint64_t n, float* xi0, float* xi1, hipStream_t s)
{
  hipLaunchKernelGGL(k_plot_draws, dim3(draw_blocks(n)), dim3(kBlock), 0, s, plot_key(seed), offset, n, xi0, xi1);
  return launched("plot draws: kernel launch failed");
}

int sphere_dirs_launch(const ImageArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(k_sphere_pixel_dirs, dim3(pixel_blocks(uint64_t(a.width) * a.height)), dim3(kBlock), 0, s, a);
  return launched("sphere directions: kernel launch failed");
}

int render_shade_launch(uint64_t npix, const float* r, const float* g, const float* b, const float* iz, const uint8_t* mask,
                        float* img, hipStream_t s)
{
  hipLaunchKernelGGL(k_render_shade, dim3(pixel_blocks(npix)), dim3(kBlock), 0, s, npix, r, g, b, iz, mask, img);
  return launched("render shade: kernel launch failed");
}

int plot_dirs_launch(const ImageArgs& a, hipStream_t s)
{
  hipLaunchKernelGGL(k_plot_light_dirs, dim3(draw_blocks(uint64_t(a.width) * a.height * a.samples)), dim3(kBlock), 0, s, a);
  return launched("plot directions: kernel launch failed");
}

int plot_accumulate_launch(const ImageArgs& a, const float* r, const float* g, const float* b, hipStream_t s)
{
  const dim3 grid(pixel_blocks(uint64_t(a.width) * a.height));
  if (a.op == kPlotEval) hipLaunchKernelGGL((k_plot_accumulate<kPlotEval>), grid, dim3(kBlock), 0, s, a, r, g, b);
  else hipLaunchKernelGGL((k_plot_accumulate<kPlotPdf>), grid, dim3(kBlock), 0, s, a, r, g, b);
  return launched("plot accumulate: kernel launch failed");
}

int plot_bin_launch(uint32_t w, uint32_t h, uint64_t n, const float* dx, const float* dy, const float* dz, const float* pdf,
                    int mask_zero, unsigned long long* counts, hipStream_t s)
{
  hipLaunchKernelGGL(k_plot_bin, dim3(draw_blocks(n)), dim3(kBlock), 0, s, w, h, n, dx, dy, dz, pdf, mask_zero, counts);
  return launched("plot bin: kernel launch failed");
}

}  // namespace bbmhip
