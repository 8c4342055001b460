// bbm_amd/csrc/registry.hip -- the model registry: one row per model name with its composition's floatRGB and
// doubleRGB launchers, attribute layout, defaults, bounds and attribute flags; and the metadata entry points of
// the C-ABI (include/bbm_hip.h) that read it.  The kernels live in kernels.hpp / f64.hpp and are instantiated in
// inst_*.hip / f64.hip; this unit only takes the launchers' addresses.
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bbm_hip.h"
#include "registry.hpp"
#include "models.hpp"

namespace bbmhip {

BBM_HIP_MICROFACET_MODELS(BBM_HIP_EXTERN)
BBM_HIP_LOBE_MODELS(BBM_HIP_EXTERN)
BBM_HIP_DIFFUSE_MODELS(BBM_HIP_EXTERN)
BBM_HIP_SPECTRAL_MODELS(BBM_HIP_EXTERN)
BBM_HIP_AGGREGATE_MODELS(BBM_HIP_EXTERN)
BBM_HIP_EPD_MODELS(BBM_HIP_EXTERN)
BBM_HIP_HE_MODELS(BBM_HIP_EXTERN)
BBM_HIP_MERL_MODELS(BBM_HIP_EXTERN)
BBM_HIP_MICROFACET_TANGENT_MODELS(BBM_HIP_EXTERN_TANGENT)
BBM_HIP_LOBE_TANGENT_MODELS(BBM_HIP_EXTERN_TANGENT)

// Merl is measured data in float: no doubleRGB kernel
template<> struct f64::has_f64<Merl> { static constexpr bool value = false; };

namespace {

template<class M> f64::F64Launchers f64_launchers()
{
  if constexpr (f64::has_f64<M>::value) return f64::f64_launchers_of<M>();
  else return {};
}

constexpr float kFMax = 3.4028234663852886e+38f;
constexpr float kFMin = 1.1754943508222875e-38f;

// One row: its name, composition M (both launcher bundles), component flags, attribute layout, then N defaults,
// lower and upper bounds and N attribute letters; N is checked against the composition here, for every row.
template<class M, int N>
ModelEntry row(const char* name, uint32_t components, const char* layout, const float (&defaults)[N],
               const float (&lower)[N], const float (&upper)[N], const char (&attrs)[N + 1])
{
  static_assert(M::kParams == N, "registry nparams must match the composition");
  ModelEntry e{name, N, components, launchers<M>(), f64_launchers<M>(), layout, {}, {}, {}, attrs, tangent_launchers<M>()};
  for (int i = 0; i < N; ++i)
  {
    e.defaults[i] = defaults[i]; e.lower[i] = lower[i]; e.upper[i] = upper[i];
  }
  return e;
}

// a second name for a row (the reference exports the same composition under both)
ModelEntry alias(const char* name, ModelEntry e)
{
  e.name = name;
  return e;
}

// Defaults and bounds: bsdf_attribute.h:73-94 (scale 0.5 in [0,1], roughness 0.1 in [0,1] as
// reported by parameter_lower_bound/upper_bound, ior 1.3 in [1,5]); pinned against
// tests/golden/models.json by tests/test_abi.py.
const ModelEntry kCookTorrance = row<CookTorranceM, 5>("CookTorrance", kFlagSpecular, "albedo:3,roughness:1,eta:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 1.3f}, {0, 0, 0, kEpsF, 1}, {1, 1, 1, 1, 5}, "ssspp");
const ModelEntry kLowMicrofacet = row<LowMicrofacetM, 6>("LowMicrofacet", kFlagSpecular, "A:3,B:1,C:1,eta:1",
   {1, 1, 1, 1, 1, 1.3f}, {0, 0, 0, 0, 0, 1}, {kFMax, kFMax, kFMax, kFMax, kFMax, 5}, "pppppp");
const ModelEntry kPhong = row<PhongLobe, 4>("Phong", kFlagSpecular, "albedo:3,sharpness:1",
   {0.5f, 0.5f, 0.5f, 32.0f}, {0, 0, 0, 0}, {1, 1, 1, kFMax}, "sssp");

// He family (bsdfmodel/he.h:473-477, :489-496): roughness, autocorrelation, eta (complex RGB: n RGB, k RGB)
template<class M> ModelEntry he_row(const char* name)
{
  return row<M, 8>(name, kFlagSpecular, "roughness:1,autocorrelation:1,eta:6", {0.18f, 3.0f, 1.3f, 1.3f, 1.3f, 0, 0, 0},
                   {0, 0, 0.1f, 0.1f, 0.1f, 0, 0, 0}, {kFMax, kFMax, 5, 5, 5, 10, 10, 10}, "pppppppp");
}

// The single models.  A model id is an index into this table followed by the aggregates, and ids cross the ABI:
// new rows go at the end, and no row moves.
const ModelEntry kSingle[] = {
  row<Lambertian, 3>("Lambertian", kFlagDiffuse, "albedo:3", {0.5f, 0.5f, 0.5f}, {0, 0, 0}, {1, 1, 1}, "ddd"),
  kCookTorrance,
  alias("LowCookTorrance", kCookTorrance),   // bsdfmodel/low.h:32-33
  row<GGXM, 5>("GGX", kFlagSpecular, "albedo:3,roughness:1,eta:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 1.3f}, {0, 0, 0, kEpsF, 1}, {1, 1, 1, 1, 5}, "ssspp"),
  row<CookTorranceWalterM, 5>("CookTorranceWalter", kFlagSpecular, "albedo:3,roughness:1,eta:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 1.3f}, {0, 0, 0, kEpsF, 1}, {1, 1, 1, 1, 5}, "ssspp"),
  row<CookTorranceHeitzM, 6>("CookTorranceHeitz", kFlagSpecular, "albedo:3,roughness:2,eta:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 0.1f, 1.3f}, {0, 0, 0, kEpsF, kEpsF, 1}, {1, 1, 1, 1, 1, 5}, "sssppp"),
  row<GGXHeitzM, 6>("GGXHeitz", kFlagSpecular, "albedo:3,roughness:2,eta:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 0.1f, 1.3f}, {0, 0, 0, kEpsF, kEpsF, 1}, {1, 1, 1, 1, 1, 5}, "sssppp"),
  row<NganCookTorranceM, 5>("NganCookTorrance", kFlagSpecular, "albedo:3,roughness:1,eta:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 0.1f}, {0, 0, 0, kEpsF, 0}, {1, 1, 1, 1, 1}, "ssspp"),
  row<PhongWalterM, 5>("PhongWalter", kFlagSpecular, "albedo:3,sharpness:1,eta:1",
   {0.5f, 0.5f, 0.5f, 32.0f, 1.3f}, {0, 0, 0, 0, 1}, {1, 1, 1, kFMax, 5}, "ssspp"),
  row<RibardiereM, 6>("Ribardiere", kFlagSpecular, "albedo:3,roughness:1,gamma:1,eta:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 2.0f, 1.3f}, {0, 0, 0, kEpsF, 1.5f + kEpsF, 1}, {1, 1, 1, 1, 40, 5}, "sssppp"),
  row<RibardiereAnisoM, 7>("RibardiereAnisotropic", kFlagSpecular, "albedo:3,roughness:2,gamma:1,eta:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 0.1f, 2.0f, 1.3f}, {0, 0, 0, kEpsF, kEpsF, 1.5f + kEpsF, 1}, {1, 1, 1, 1, 1, 40, 5}, "ssspppp"),
  row<OrenNayar, 4>("OrenNayar", kFlagDiffuse, "albedo:3,roughness:1",
   {0.5f, 0.5f, 0.5f, 0.1f}, {0, 0, 0, kEpsF}, {1, 1, 1, 1}, "dddD"),
  kLowMicrofacet,
  alias("LowMicrofacetFit", kLowMicrofacet),
  row<WardM, 5>("Ward", kFlagSpecular, "albedo:3,roughness:2",
   {0.5f, 0.5f, 0.5f, 0.1f, 0.1f}, {0, 0, 0, kEpsF, kEpsF}, {1, 1, 1, 1, 1}, "ssspp"),
  row<WardDuerM, 5>("WardDuer", kFlagSpecular, "albedo:3,roughness:2",
   {0.5f, 0.5f, 0.5f, 0.1f, 0.1f}, {0, 0, 0, kEpsF, kEpsF}, {1, 1, 1, 1, 1}, "ssspp"),
  row<WardDGMM, 5>("WardDuerGeislerMoroder", kFlagSpecular, "albedo:3,roughness:2",
   {0.5f, 0.5f, 0.5f, 0.1f, 0.1f}, {0, 0, 0, kEpsF, kEpsF}, {1, 1, 1, 1, 1}, "ssspp"),
  row<NganWardM, 4>("NganWard", kFlagSpecular, "albedo:3,roughness:1",
   {0.5f, 0.5f, 0.5f, 0.1f}, {0, 0, 0, kEpsF}, {1, 1, 1, 1}, "sssp"),
  row<NganWardDuerM, 4>("NganWardDuer", kFlagSpecular, "albedo:3,roughness:1",
   {0.5f, 0.5f, 0.5f, 0.1f}, {0, 0, 0, kEpsF}, {1, 1, 1, 1}, "sssp"),
  kPhong,
  alias("NganBlinnPhong", kPhong),   // ngan.h:43-44
  row<LafortuneM, 7>("Lafortune", kFlagSpecular, "albedo:3,Cxy:2,Cz:1,sharpness:1",
   {0.5f, 0.5f, 0.5f, -0.57735026919f, -0.57735026919f, 0.57735026919f, 32.0f},
   {0, 0, 0, kFMin, kFMin, kFMin, 0}, {1, 1, 1, kFMax, kFMax, kFMax, kFMax}, "ssspppp"),
  row<NganLafortuneM, 6>("NganLafortune", kFlagSpecular, "albedo:3,Cxy:1,Cz:1,sharpness:1",
   {0.5f, 0.5f, 0.5f, -0.57735026919f, 0.57735026919f, 32.0f}, {0, 0, 0, kFMin, kFMin, 0}, {1, 1, 1, kFMax, kFMax, kFMax}, "sssppp"),
  row<ASM, 5>("AshikhminShirley", kFlagSpecular, "fresnelReflectance:3,sharpness:2",
   {0.1f, 0.1f, 0.1f, 32.0f, 32.0f}, {0, 0, 0, 0, 0}, {1, 1, 1, kFMax, kFMax}, "ppppp"),
  row<ASFullM, 8>("AshikhminShirleyFull", kFlagAll, "diffuseReflectance:3,fresnelReflectance:3,sharpness:2",
   {0.5f, 0.5f, 0.5f, 0.1f, 0.1f, 0.1f, 32.0f, 32.0f}, {0, 0, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 1, kFMax, kFMax}, "dddppppp"),
  row<LowASM, 5>("LowAshikhminShirley", kFlagSpecular, "albedo:3,fresnelReflectance:1,sharpness:1",
   {0.5f, 0.5f, 0.5f, 1.3f, 32.0f}, {0, 0, 0, 1, 0}, {1, 1, 1, 5, kFMax}, "ssspp"),
  row<NganASM, 5>("NganAshikhminShirley", kFlagSpecular, "albedo:3,fresnelReflectance:1,sharpness:1",
   {0.5f, 0.5f, 0.5f, 0.1f, 32.0f}, {0, 0, 0, 0, 0}, {1, 1, 1, 1, kFMax}, "ssspp"),
  row<LowSmooth, 6>("LowSmooth", kFlagSpecular, "A:3,B:1,C:1,eta:1",
   {1, 1, 1, 1, 1, 1.3f}, {0, 0, 0, 0, 0, 1}, {kFMax, kFMax, kFMax, kFMax, kFMax, 5}, "pppppp"),
  // bsdfmodel/bagher.h:62-68: albedo, K, Lambda, c, theta0, k (ndf/sgd.h:197-203, Dependent),
  // alpha, p (sgd.h:107-111), eta = (F0, F1) RGB (bagher.h:31, default {1, 0}, lower {0, -1})
  row<Bagher, 30>("Bagher", kFlagSpecular, "albedo:3,K:3,Lambda:3,c:3,theta0:3,k:3,alpha:3,p:3,eta:6",
   {0.5f, 0.5f, 0.5f, 7.5f, 7.5f, 7.5f, 1, 1, 1, 1, 1, 1, 1.5707963705062866f, 1.5707963705062866f, 1.5707963705062866f,
    1, 1, 1, 0.1f, 0.1f, 0.1f, 0.64f, 0.64f, 0.64f, 1, 1, 1, 0, 0, 0},
   {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, kEpsF, kEpsF, kEpsF, 0, 0, 0, 0, 0, 0, -1, -1, -1},
   {1, 1, 1, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax, kFMax,
    1, 1, 1, kFMax, kFMax, kFMax, 1, 1, 1, 1, 1, 1}, "sssxxxxxxxxxxxxxxxpppppppppppp"),
  // EPD (bsdfmodel/holzschuchpacanowski.h:34-42): beta, p (ndf/epd.h:180-182), eta = complex ior (n, k)
  row<EpdM, 4>("EPD", kFlagSpecular, "beta:1,p:1,eta:2",
   {0.003f, 0.2f, 1.3f, 0.0f}, {0.0f, 0.0f, 0.1f, 0.0f}, {0.5f, 5.0f, 5.0f, 10.0f}, "pppp"),
  he_row<HeM>("He"),
  he_row<HeWestinM>("HeWestin"),
  he_row<HeHolzschuchM>("HeHolzschuch"),
  // ngan.h:166-167: albedo first and a scalar ior
  row<NganHeM, 6>("NganHe", kFlagSpecular, "albedo:3,roughness:1,autocorrelation:1,eta:1",
   {0.5f, 0.5f, 0.5f, 0.18f, 3.0f, 1.3f}, {0, 0, 0, 0, 0, 1}, {1, 1, 1, kFMax, kFMax, 5}, "sssppp"),
  // Merl (staticmodel/merl.h:224-225): no attributes in the reference (the data comes from a file); the two
  // slots hold the device address of a table built by bbm_hip_merl_table, flagged Dependent so no fit moves them
  row<Merl, 2>("Merl", kFlagAll, nullptr, {0, 0}, {0, 0}, {0, 0}, "xx"),
};
constexpr int kNumSingle = int(sizeof(kSingle) / sizeof(kSingle[0]));

// Aggregate(Lambertian, X) (aggregatemodel.h:22-233): parameters, defaults, bounds and attribute
// flags are Lambertian's followed by X's; `child` names the registry entry X.
struct AggregateSpec
{
  const char* name;
  const char* child;
  uint32_t components;
  Launchers run;
  f64::F64Launchers run_f64;
};
template<class M> AggregateSpec agg(const char* key, const char* child)
{
  return {key, child, kFlagDiffuse | M::kComponent, launchers<M>(), f64_launchers<M>()};
}
const AggregateSpec kAggregates[] = {
  agg<AggBagherM>("Aggregate<Lambertian,Bagher>", "Bagher"),                      // fits/bagher_sgd.fit
  agg<AggCookTorranceM>("Aggregate<Lambertian,CookTorrance>", "CookTorrance"),    // docs/source/fitting.rst:31-33
  agg<AggGGXM>("Aggregate<Lambertian,GGX>", "GGX"),
  agg<AggCookTorranceM>("Aggregate<Lambertian,LowCookTorrance>", "LowCookTorrance"),   // fits/low_cooktorrance_E*.fit
  agg<AggLowASM>("Aggregate<Lambertian,LowAshikhminShirley>", "LowAshikhminShirley"),  // fits/low_ashikhminshirley_E*.fit
  agg<AggLowMicrofacetM>("Aggregate<Lambertian,LowMicrofacetFit>", "LowMicrofacetFit"),  // fits/low_lowmicrofacet_E2.fit
  agg<AggLowSmoothM>("Aggregate<Lambertian,LowSmooth>", "LowSmooth"),             // fits/low_lowsmooth_E2.fit
  agg<AggNganASM>("Aggregate<Lambertian,NganAshikhminShirley>", "NganAshikhminShirley"),  // fits/ngan_ashikhminshirley.fit
  agg<AggPhongM>("Aggregate<Lambertian,NganBlinnPhong>", "NganBlinnPhong"),       // fits/ngan_blinnphong.fit
  agg<AggNganCookTorranceM>("Aggregate<Lambertian,NganCookTorrance>", "NganCookTorrance"),  // fits/ngan_cooktorrance.fit
  agg<AggNganLafortuneM>("Aggregate<Lambertian,NganLafortune>", "NganLafortune"),  // fits/ngan_lafortune.fit
  agg<AggNganWardM>("Aggregate<Lambertian,NganWard>", "NganWard"),                 // fits/ngan_ward.fit
  agg<AggNganWardDuerM>("Aggregate<Lambertian,NganWardDuer>", "NganWardDuer"),     // fits/ngan_wardduer.fit
  agg<AggNganHeM>("Aggregate<Lambertian,NganHe>", "NganHe"),                       // fits/ngan_he.fit
};

const ModelEntry* single(const char* name)
{
  for (const auto& e : kSingle)
    if (std::strcmp(e.name, name) == 0) return &e;
  return nullptr;
}

struct Registry
{
  std::vector<ModelEntry> models;
  std::vector<std::string> attrs;   // storage for the aggregates' attribute strings
  Registry()
  {
    models.assign(kSingle, kSingle + kNumSingle);
    const ModelEntry* lam = single("Lambertian");
    attrs.reserve(sizeof(kAggregates) / sizeof(kAggregates[0]));
    for (const auto& g : kAggregates)
    {
      const ModelEntry* c = single(g.child);
      ModelEntry e{};
      e.name = g.name;
      e.nparams = lam->nparams + c->nparams;
      e.components = g.components;
      e.run = g.run;
      e.run_f64 = g.run_f64;
      for (int i = 0; i < lam->nparams; ++i)
      {
        e.defaults[i] = lam->defaults[i]; e.lower[i] = lam->lower[i]; e.upper[i] = lam->upper[i];
      }
      for (int i = 0; i < c->nparams; ++i)
      {
        e.defaults[lam->nparams + i] = c->defaults[i];
        e.lower[lam->nparams + i] = c->lower[i];
        e.upper[lam->nparams + i] = c->upper[i];
      }
      attrs.push_back(std::string(lam->attrs) + c->attrs);
      e.attrs = attrs.back().c_str();
      models.push_back(e);
    }
  }
};

const Registry& registry()
{
  static const Registry r;
  return r;
}

int num_models() { return int(registry().models.size()); }

int unknown_id(int model_id) { return fail(BBM_HIP_ERR_INVALID_MODEL, "unknown model id " + std::to_string(model_id)); }

}  // namespace

bool runtime_id(int id) { return id >= 0 && (id & BBM_HIP_RUNTIME_AGGREGATE) != 0; }

const ModelEntry* entry(int id)
{
  const int base = (id >= 0) ? (id & ~(BBM_HIP_RUNTIME_AGGREGATE | BBM_HIP_CALL_EXACT | BBM_HIP_CALL_DEFAULT)) : id;
  if (base < 0 || base >= num_models()) return nullptr;
  const ModelEntry* e = &registry().models[size_t(base)];
  if (runtime_id(id) && base < kNumSingle) return nullptr;    // the flag applies to fused aggregates only
  return e;
}

int checked_entry(int model_id, int nparams, const void* params, bool check_params, bool f64, const ModelEntry*& e)
{
  e = entry(model_id);
  if (!e) return unknown_id(model_id);
  if (f64 && !e->run_f64.eval_pdf) return fail(BBM_HIP_ERR_UNSUPPORTED, std::string(e->name) + ": no doubleRGB kernel");
  if (nparams != e->nparams)
    return fail(BBM_HIP_ERR_INVALID_ARG, std::string(e->name) + ": expected " + std::to_string(e->nparams) +
                                             " parameters, got " + std::to_string(nparams));
  if (check_params && nparams > 0 && !params) return fail(BBM_HIP_ERR_INVALID_ARG, "params is NULL");
  return BBM_HIP_OK;
}

}  // namespace bbmhip

using namespace bbmhip;

extern "C" {

int bbm_hip_num_models(void) { return num_models(); }

const char* bbm_hip_model_name(int model_id)
{
  const ModelEntry* e = entry(model_id);
  return e ? e->name : nullptr;
}

int bbm_hip_model_id(const char* name)
{
  if (!name) return fail(BBM_HIP_ERR_INVALID_ARG, "name is NULL");
  for (int i = 0; i < num_models(); ++i)
    if (std::strcmp(registry().models[size_t(i)].name, name) == 0) return i;
  return fail(BBM_HIP_ERR_INVALID_MODEL, std::string("unknown BSDF model: ") + name);
}

int bbm_hip_model_nparams(int model_id)
{
  const ModelEntry* e = entry(model_id);
  return e ? e->nparams : unknown_id(model_id);
}

int bbm_hip_model_params(int model_id, int which, float* out, int capacity)
{
  const ModelEntry* e = entry(model_id);
  if (!e) return unknown_id(model_id);
  const float* src = (which == 0) ? e->defaults : (which == 1) ? e->lower : (which == 2) ? e->upper : nullptr;
  if (!src) return fail(BBM_HIP_ERR_INVALID_ARG, "which must be 0 (default), 1 (lower) or 2 (upper)");
  for (int i = 0; out && i < e->nparams && i < capacity; ++i) out[i] = src[i];
  return e->nparams;
}

int bbm_hip_model_components(int model_id)
{
  const ModelEntry* e = entry(model_id);
  return e ? int(e->components) : unknown_id(model_id);
}

int bbm_hip_model_param_attrs(int model_id, uint32_t* out, int capacity)
{
  const ModelEntry* e = entry(model_id);
  if (!e) return unknown_id(model_id);
  for (int i = 0; out && i < e->nparams && i < capacity; ++i)
  {
    switch (e->attrs[i])
    {
      case 'd': out[i] = 0x01u; break;
      case 'D': out[i] = 0x02u; break;
      case 's': out[i] = 0x04u; break;
      case 'p': out[i] = 0x08u; break;
      default: out[i] = 0x10u; break;
    }
  }
  return e->nparams;
}

int bbm_hip_model_has_f64(int model_id)
{
  const ModelEntry* e = entry(model_id);
  if (!e) return unknown_id(model_id);
  return e->run_f64.eval_pdf ? 1 : 0;
}

int bbm_hip_model_has_varying(int model_id)
{
  const ModelEntry* e = entry(model_id);
  if (!e) return unknown_id(model_id);
  return e->run.eval_pdf_var ? 1 : 0;
}

int bbm_hip_model_has_table(int model_id)
{
  const ModelEntry* e = entry(model_id);
  if (!e) return unknown_id(model_id);
  return e->run.eval_pdf_tab ? 1 : 0;
}

int bbm_hip_model_anisotropic(int model_id)
{
  const ModelEntry* e = entry(model_id);
  if (!e) return unknown_id(model_id);
  return e->tangent.eval_pdf ? 1 : 0;
}

const char* bbm_hip_model_layout(int model_id)
{
  const ModelEntry* e = entry(model_id);
  if (!e) { unknown_id(model_id); return nullptr; }
  return e->layout;
}

}  // extern "C"
