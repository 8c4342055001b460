// bbm_amd/csrc/table.hpp -- material tables: one launch over many parameter sets of one model, selected per lane by
// a 4-byte index (bbm_hip_table_*, bbm_hip_eval_pdf_table / _sample_table / _reflectance_table).
// Included at the end of kernels.hpp, after varying.hpp: the table source of the per-lane kernels (lanes.hpp).
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
// The quad form loads the quad's four indices as one 16-byte nontemporal vector; a lane's gather is a few aligned
// 16-byte loads of its material's block (lanes.hpp has the kernels).
#pragma once

namespace bbmhip {

// Slots of the parameter block a model's constructor reads, counted from slot 0 (the fused aggregates' mode slot,
// kMaxParams - 1, aside): its own parameters, and what host_params appends for it.  Specialised in models.hpp.
template<class Model> struct table_slots { static constexpr int value = Model::kParams; };

// floats between two materials' blocks: the slots rounded up to whole 16-byte loads
constexpr int table_stride(int slots) { return (slots + 3) & ~3; }

// Whether the fused quad form is used for aligned arrays (from the compiler's resource report)
template<class Model> struct tab_quad { static constexpr bool value = true; };

// A table and a call's indices into it: a lane-parameter source (lanes.hpp).
struct TabRef
{
  const float* blocks;         // count x stride floats, 16-byte aligned
  const uint32_t* material;    // n indices
  uint32_t count;

  // the blocks were prepared at create (table_prepare); the kernarg block is the fallback, material 0's
  static constexpr bool kHostPrepare = false;
  template<class Model> static constexpr int slots = table_slots<Model>::value;
  template<class Model> static constexpr bool quad = tab_quad<Model>::value;

  bool aligned(int) const { return aligned16(material); }

  template<int S> struct Quad { uint32_t id[4]; };

  template<int S> __device__ __forceinline__ Quad<S> load_quad(uint64_t t) const
  {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4 idv = __builtin_nontemporal_load(reinterpret_cast<const u4*>(material) + t);
    return {{idv.x, idv.y, idv.z, idv.w}};
  }

  // Material `id`'s block: the fallback `u` with the model's slots replaced by the table's where id is in range.
  // Nothing is loaded for an id out of range, and the lane is then not live.  The loop bound is a compile-time
  // constant and every index a constant after unrolling, so the block lives in registers and only the slots the
  // constructor reads are loaded.
  template<int S> __device__ __forceinline__ void block(const ParamBlock& u, uint32_t id, ParamBlock& q) const
  {
#pragma unroll
    for (int k = 0; k < kMaxParams; ++k) q.v[k] = u.v[k];
    if (id < count)
    {
      const float* row = static_cast<const float*>(
          __builtin_assume_aligned(blocks + size_t(id) * size_t(table_stride(S)), 16));
#pragma unroll
      for (int k = 0; k < S; ++k) q.v[k] = row[k];
    }
  }

  template<int S>
  __device__ __forceinline__ void quad_block(const ParamBlock& u, const Quad<S>& c, int j, ParamBlock& q) const
  {
    block<S>(u, c.id[j], q);
  }
  template<int S> __device__ __forceinline__ bool quad_live(const Quad<S>& c, int j) const { return c.id[j] < count; }

  // lane i on its own (the one-lane kernels and the quad kernels' tail): its index
  struct Lane { uint32_t id; };
  __device__ __forceinline__ Lane load_lane(uint64_t i) const { return {material[i]}; }
  template<int S> __device__ __forceinline__ void lane_block(const ParamBlock& u, Lane l, uint64_t, ParamBlock& q) const
  {
    block<S>(u, l.id, q);
  }
  __device__ __forceinline__ bool lane_live(Lane l) const { return l.id < count; }
};

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

}  // namespace bbmhip
