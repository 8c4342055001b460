// bbm_amd/csrc/table.hpp -- material tables: one launch over many parameter sets of one model, selected per lane by
// a 4-byte index (bbm_hip_table_*, bbm_hip_eval_pdf_table / _sample_table / _reflectance_table).
// Included at the end of kernels.hpp, after varying.hpp.
//
// A table is `count` prepared parameter blocks in device memory, `stride` floats apart.  A block is what the uniform
// entry point passes in its kernarg for that material -- the raw parameters followed by whatever host_params writes
// behind them (EPD's tgammaf slots) -- cut to the slots the model's constructor reads (table_slots) and padded to a
// multiple of four floats, so a lane's gather is a few aligned 16-byte loads and a 5-parameter material costs 32 B
// of cache, not a 256 B ParamBlock.  The uniform entry points run host_params only where a pdf is asked for (eval +
// pdf, pdf, sample), not for eval alone or reflectance; where host_params changes the block (EPD) the table therefore
// keeps both forms, and each call reads the one its uniform twin would see.  A fused aggregate's mode slot
// (BBM_HIP_RUNTIME_AGGREGATE, baked in at create) is the same for every material and rides in the kernarg block.
//
// Lane i builds `const Model m(block)` from material[i]'s block and calls the device functions the uniform kernels
// call (model_eval_pdf, one_sample, reflectance): its result is the uniform kernel's for that material, bit for
// bit.  A lane whose index is >= count loads nothing: it takes the kernarg block (material 0's, the fallback) with
// the component cleared, which is what a lane with mask[i] == 0 is to the uniform kernels.
//
// Layout of the eval kernel: k_eval_pdf_v4's -- four consecutive pairs per thread, one 16-byte nontemporal load per
// direction array and one for the quad's four indices, 16-byte nontemporal stores, a scalar tail -- with the model
// built inside the j loop, so one model is live at a time.  Unaligned arrays take one pair per thread
// (k_eval_pdf_tab1); sample and reflectance run one lane per thread.  All grids are full.
#pragma once

namespace bbmhip {

// Slots of the parameter block a model's constructor reads, counted from slot 0 (the fused aggregates' mode slot,
// kMaxParams - 1, aside): its own parameters, and what host_params appends for it.  Specialised in models.hpp.
template<class Model> struct table_slots { static constexpr int value = Model::kParams; };

// floats between two materials' blocks: the slots rounded up to whole 16-byte loads
constexpr int table_stride(int slots) { return (slots + 3) & ~3; }

// Whether the fused quad form is used for aligned arrays (from the compiler's resource report)
template<class Model> struct tab_quad { static constexpr bool value = true; };

struct TabRef
{
  const float* blocks;         // count x stride floats, 16-byte aligned
  const uint32_t* material;    // n indices
  uint32_t count;
};

struct EvalTabArgs { EvalArgs e; TabRef t; };      // e.p: the fallback block (and the aggregate mode slot)
struct SampleTabArgs { SampleArgs e; TabRef t; };
struct ReflTabArgs { ReflArgs e; TabRef t; };

// Material `id`'s block: the fallback `u` with the model's slots replaced by the table's where id is in range.
// Nothing is loaded for an id out of range.  The loop bound is a compile-time constant and every index a constant
// after unrolling, so the block lives in registers and only the slots the constructor reads are loaded.
template<int S>
__device__ __forceinline__ void tab_block(const ParamBlock& u, const TabRef& t, uint32_t id, ParamBlock& q)
{
#pragma unroll
  for (int k = 0; k < kMaxParams; ++k) q.v[k] = u.v[k];
  if (id < t.count)
  {
    const float* row = static_cast<const float*>(
        __builtin_assume_aligned(t.blocks + size_t(id) * size_t(table_stride(S)), 16));
#pragma unroll
    for (int k = 0; k < S; ++k) q.v[k] = row[k];
  }
}

template<class Model, int MODE, bool EXACT>
__device__ __forceinline__ void tab_one_pair(const EvalTabArgs& a, uint64_t i)
{
  const EvalArgs& e = a.e;
  const uint32_t id = a.t.material[i];
  ParamBlock q;
  tab_block<table_slots<Model>::value>(e.p, a.t, id, q);
  const Model m(q.v);
  float rgb[3], pdf;
  const bool active = (e.mask ? (e.mask[i] != 0) : true) && id < a.t.count;
  model_eval_pdf<MODE, EXACT>(m, mk3(e.ix[i], e.iy[i], e.iz[i]), mk3(e.ox[i], e.oy[i], e.oz[i]),
                              active ? e.component : 0u, rgb, pdf);
  if (MODE & kModeEval) { e.r[i] = rgb[0]; e.g[i] = rgb[1]; e.b[i] = rgb[2]; }
  if (MODE & kModePdf) e.pdf[i] = pdf;
}

// Four pairs per thread; every float array and the index array 16-byte aligned, the mask 4-byte aligned.
template<class Model, int MODE, bool EXACT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(eval_waves<Model>::value, 8)))
void k_eval_pdf_tab(EvalTabArgs a)
{
  math_tables_init();
  const EvalArgs& e = a.e;
  const uint64_t n4 = e.n >> 2;
  const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t < n4)
  {
    const float4 ix = ld4<true>(e.ix, t), iy = ld4<true>(e.iy, t), iz = ld4<true>(e.iz, t);
    const float4 ox = ld4<true>(e.ox, t), oy = ld4<true>(e.oy, t), oz = ld4<true>(e.oz, t);
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4 idv = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a.t.material) + t);
    const uint32_t mk = e.mask ? reinterpret_cast<const uint32_t*>(e.mask)[t] : 0x01010101u;
    const uint32_t id[4] = {idv.x, idv.y, idv.z, idv.w};
    const float inx[4] = {ix.x, ix.y, ix.z, ix.w}, iny[4] = {iy.x, iy.y, iy.z, iy.w}, inz[4] = {iz.x, iz.y, iz.z, iz.w};
    const float onx[4] = {ox.x, ox.y, ox.z, ox.w}, ony[4] = {oy.x, oy.y, oy.z, oy.w}, onz[4] = {oz.x, oz.y, oz.z, oz.w};
    float r[4], g[4], b[4], p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      ParamBlock q;
      tab_block<table_slots<Model>::value>(e.p, a.t, id[j], q);
      const Model m(q.v);
      float rgb[3];
      const uint32_t comp = (((mk >> (8 * j)) & 0xffu) && id[j] < a.t.count) ? e.component : 0u;
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
  if (blockIdx.x == 0 && threadIdx.x < (e.n & 3)) tab_one_pair<Model, MODE, EXACT>(a, (n4 << 2) + threadIdx.x);
}

// One pair per thread: unaligned arrays (and the rows tab_quad excludes).
template<class Model, int MODE, bool EXACT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(eval_waves<Model>::value, 8)))
void k_eval_pdf_tab1(EvalTabArgs a)
{
  math_tables_init();
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i < a.e.n) tab_one_pair<Model, MODE, EXACT>(a, i);
}

// S: the slot count of the model the table was made for (Model may be its exact-mode sampling twin)
template<class Model, int S>
__global__ __launch_bounds__(kBlock) void k_sample_tab(SampleTabArgs a)
{
  math_tables_init();
  const SampleArgs& e = a.e;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= e.n) return;
  const uint32_t id = a.t.material[i];
  ParamBlock q;
  tab_block<S>(e.p, a.t, id, q);
  const Model m(q.v);
  one_sample<Model>(m, e, i, (e.mask ? (e.mask[i] != 0) : true) && id < a.t.count);
}

template<class Model>
__global__ __launch_bounds__(kBlock) void k_reflectance_tab(ReflTabArgs a)
{
  math_tables_init();
  const ReflArgs& e = a.e;
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= e.n) return;
  const uint32_t id = a.t.material[i];
  ParamBlock q;
  tab_block<table_slots<Model>::value>(e.p, a.t, id, q);
  const Model m(q.v);
  float rgb[3];
  const bool active = (e.mask ? (e.mask[i] != 0) : true) && id < a.t.count;
  m.reflectance(mk3(e.ox[i], e.oy[i], e.oz[i]), active ? e.component : 0u, rgb);
  e.r[i] = rgb[0]; e.g[i] = rgb[1]; e.b[i] = rgb[2];
}

// What bbm_hip_table_create runs per material, on the host: the checks and derived data of the uniform entry points
// (host_prepare once per table, host_validate, host_params), giving the block as eval-alone / reflectance see it
// (`raw`) and as eval + pdf / pdf / sample see it (`prepared`), and the model's slot count.
struct TableBlocks { ParamBlock raw, prepared; int slots; };

template<class Model>
int table_prepare(const ParamBlock& in, bool first, hipStream_t s, TableBlocks& out)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    if (first)
      if (const int rc = host_prepare<Model>::run(s)) return rc;
    if (const int rc = host_validate<Model>::run(in)) return rc;
    out.raw = in;
    out.prepared = in;
    out.slots = table_slots<Model>::value;
    void* scratch = nullptr;
    const int rc = host_params<Model>::run(out.prepared, kFlagAll, s, &scratch);
    host_params<Model>::done(scratch, s);
    if (rc) return rc;
    // what the kernels do not gather must not differ between materials: nothing beyond the model's slots
    for (int k = out.slots; k < kMaxParams - 1; ++k)
      if (out.prepared.v[k] != 0.0f || out.raw.v[k] != 0.0f)
        return fail(BBM_HIP_ERR_UNSUPPORTED, "material table: the model's block has data beyond its table slots");
    return BBM_HIP_OK;
  }
}

template<class Model, int MODE, bool EXACT>
int launch_tab_mode(const EvalTabArgs& a, hipStream_t s)
{
  const EvalArgs& e = a.e;
  bool vec = tab_quad<Model>::value && aligned16(e.ix) && aligned16(e.iy) && aligned16(e.iz) && aligned16(e.ox) &&
             aligned16(e.oy) && aligned16(e.oz) && (reinterpret_cast<uintptr_t>(e.mask) & 3u) == 0 &&
             aligned16(a.t.material);
  if (MODE & kModeEval) vec = vec && aligned16(e.r) && aligned16(e.g) && aligned16(e.b);
  if (MODE & kModePdf) vec = vec && aligned16(e.pdf);
  const unsigned blocks = var_blocks(vec ? (e.n >> 2) : e.n);
  if (blocks == 0) return var_launched(blocks);
  if constexpr (tab_quad<Model>::value)
  {
    if (vec) hipLaunchKernelGGL((k_eval_pdf_tab<Model, MODE, EXACT>), dim3(blocks), dim3(kBlock), 0, s, a);
  }
  if (!vec) hipLaunchKernelGGL((k_eval_pdf_tab1<Model, MODE, EXACT>), dim3(blocks), dim3(kBlock), 0, s, a);
  return var_launched(blocks);
}

template<class Model, int MODE>
int launch_tab_exact(const EvalTabArgs& a, hipStream_t s)
{
  if constexpr (model_has_exact<Model>())
    if (exact_on()) return launch_tab_mode<Model, MODE, true>(a, s);
  return launch_tab_mode<Model, MODE, false>(a, s);
}

template<class Model>
int launch_eval_pdf_tab(const EvalTabArgs& a, int mode, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    switch (mode)
    {
      case kModeEval: return launch_tab_exact<Model, kModeEval>(a, s);
      case kModePdf: return launch_tab_exact<Model, kModePdf>(a, s);
      default: return launch_tab_exact<Model, kModeEvalPdf>(a, s);
    }
  }
}

template<class Model>
int launch_sample_tab(const SampleTabArgs& a, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    const unsigned blocks = var_blocks(a.e.n);
    if (blocks == 0) return var_launched(blocks);
    constexpr int S = table_slots<Model>::value;
    bool twin = false;
    if constexpr (has_exact_sample<Model>())       // exact mode: the sampler's twin (launch_sample_mask)
      if (exact_on())
      {
        hipLaunchKernelGGL((k_sample_tab<exact_sample_t<Model>, S>), dim3(blocks), dim3(kBlock), 0, s, a);
        twin = true;
      }
    if (!twin) hipLaunchKernelGGL((k_sample_tab<Model, S>), dim3(blocks), dim3(kBlock), 0, s, a);
    return var_launched(blocks);
  }
}

template<class Model>
int launch_reflectance_tab(const ReflTabArgs& a, hipStream_t s)
{
  if constexpr (!supports_varying<Model>::value) return var_unsupported();
  else
  {
    const unsigned blocks = var_blocks(a.e.n);
    if (blocks == 0) return var_launched(blocks);
    hipLaunchKernelGGL((k_reflectance_tab<Model>), dim3(blocks), dim3(kBlock), 0, s, a);
    return var_launched(blocks);
  }
}

}  // namespace bbmhip
