// bbm_amd/csrc/models.hpp -- the model compositions the library implements (one line per
// reference model, file:line of its definition), and the X-macro lists the instantiation units
// and the registry iterate over.
#pragma once
#include "diffuse.hpp"
#include "lobes.hpp"
#include "microfacet.hpp"
#include "spectral.hpp"
#include "aggregate.hpp"
#include "epd.hpp"
#include "he.hpp"
#include "merl.hpp"

#include <type_traits>

namespace bbmhip {

// Launch traits of the eval kernels (kernels.hpp), specialised here where every model type is complete.
// Aggregate(Lambertian, X) is zero outside the upper hemisphere and on masked lanes whenever X is (Lambertian's
// eval and pdf both need z(in), z(out) > 0), so it shares X's compaction and occupancy choices.
template<class B> struct compact_eval<Aggregate<Lambertian, B>> { static constexpr bool value = compact_eval<B>::value; };
template<class B> struct eval_waves<Aggregate<Lambertian, B>> { static constexpr int value = eval_waves<B>::value; };
template<class B> struct loss_waves<Aggregate<Lambertian, B>> { static constexpr int value = loss_waves<B>::value; };
template<class B> struct eval_grid_cap<Aggregate<Lambertian, B>> { static constexpr uint64_t value = eval_grid_cap<B>::value; };
template<class B> struct eval_prefetch<Aggregate<Lambertian, B>> { static constexpr bool value = eval_prefetch<B>::value; };
template<class FRES, bool ERRATA, bool WESTIN, int TAYLOR, bool ADAPTIVE, int APPROX, bool SCALED>
struct loss_waves<He<FRES, ERRATA, WESTIN, TAYLOR, ADAPTIVE, APPROX, SCALED>> { static constexpr int value = 1; };
template<class B> struct loss_pair_waves<Aggregate<Lambertian, B>> { static constexpr int value = loss_pair_waves<B>::value; };
template<class B> struct check_waves<Aggregate<Lambertian, B>> { static constexpr int value = check_waves<B>::value; };
template<class FRES, bool ERRATA, bool WESTIN, int TAYLOR, bool ADAPTIVE, int APPROX, bool SCALED>
struct check_waves<He<FRES, ERRATA, WESTIN, TAYLOR, ADAPTIVE, APPROX, SCALED>> { static constexpr int value = 1; };
template<> struct check_waves<EpdM> { static constexpr int value = 1; };
template<class FRES, bool ERRATA, bool WESTIN, int TAYLOR, bool ADAPTIVE, int APPROX, bool SCALED>
struct loss_pair_waves<He<FRES, ERRATA, WESTIN, TAYLOR, ADAPTIVE, APPROX, SCALED>> { static constexpr int value = 1; };
// Per-lane parameters (varying.hpp): not the He family, whose sample / pdf read a CDF built per launch from the
// parameters, nor Merl, which has a table address and no parameters; an aggregate follows its second child.
template<class FRES, bool ERRATA, bool WESTIN, int TAYLOR, bool ADAPTIVE, int APPROX, bool SCALED>
struct supports_varying<He<FRES, ERRATA, WESTIN, TAYLOR, ADAPTIVE, APPROX, SCALED>> { static constexpr bool value = false; };
template<> struct supports_varying<Merl> { static constexpr bool value = false; };
template<class B> struct supports_varying<Aggregate<Lambertian, B>> { static constexpr bool value = supports_varying<B>::value; };
// Material tables (table.hpp): the slots a block keeps per material.  EPD's constructor also reads the two slots
// host_params<EpdM> writes behind its parameters; an aggregate's block is its children's, one after the other.
template<> struct table_slots<EpdM> { static constexpr int value = EpdM::kParams + 2; };
template<class B> struct table_slots<Aggregate<Lambertian, B>> { static constexpr int value = Lambertian::kParams + table_slots<B>::value; };
// Bagher's fitting loss (config 5) runs at 8 waves per SIMD: 64 VGPRs with ~55 of the per-sample decode state spilled
// to scratch (read back once per probe pair from L1), against 128 VGPRs and no spills at 4.  The kernel is
// latency-bound (issue 0.40), so the doubled occupancy outweighs the spill traffic.  Measured on config 5, ms per
// compass step, interleaved (profiles/r04_ab_fit_loss_waves*.txt): 4 waves 0.591, 5 0.618, 6 0.572, 7 0.588,
// 8 0.554; at 8 waves 3 or 4 probes per iteration 0.559 / 0.567, the probe models staged in LDS 0.566.
#ifndef BBM_HIP_BAGHER_LOSS_WAVES
#define BBM_HIP_BAGHER_LOSS_WAVES 8
#endif
template<> struct loss_pair_waves<Bagher> { static constexpr int value = BBM_HIP_BAGHER_LOSS_WAVES; };
// Bagher's evaluation holds ~180 VGPRs (two waves per SIMD) unconstrained.  Measured (10M pairs, eval+pdf,
// tools/gpu_ab_he.sh): Bagher 0.238 / 0.203 / 0.262 ms and Aggregate(Lambertian, Bagher) 0.266 / 0.231 / 0.324 ms
// at 2 / 3 / 4 waves per SIMD -- three it is.
#ifndef BBM_HIP_BAGHER_WAVES
#define BBM_HIP_BAGHER_WAVES 3
#endif
template<> struct eval_waves<Bagher> { static constexpr int value = BBM_HIP_BAGHER_WAVES; };
template<> struct eval_prefetch<Bagher> { static constexpr bool value = false; };
#ifdef BBM_HIP_BAGHER_COMPACT
template<> struct compact_eval<Bagher> { static constexpr bool value = true; };   // A/B
#endif
#ifdef BBM_HIP_MERL_WAVES
template<> struct eval_waves<Merl> { static constexpr int value = BBM_HIP_MERL_WAVES; };   // A/B
#endif
#ifdef BBM_HIP_EPD_WAVES
template<> struct eval_waves<EpdM> { static constexpr int value = BBM_HIP_EPD_WAVES; };   // A/B
#endif

// Ribardiere's per-thread Student-T setup (two tgamma, a pow): 2048 workgroups (8 per CU, each thread ~5 iterations
// over 10M pairs) measured 0.139 -> 0.121 ms per 10M-pair eval (1024 / 4096 / 8192: 0.125 / 0.128 / 0.134;
// tools/gpu_ab_blocks.sh); the HBM-bound models lose 5-15 % under the same cap and keep the full grid.

// Compositions (reference file:line):
using CookTorranceM = Microfacet<Beckmann<false, false>, VGroove, FresnelCook, Norm::Cook, true>;         // bsdfmodel/cooktorrance.h:28-34
#ifdef BBM_HIP_CT_WAVES
template<> struct eval_waves<CookTorranceM> { static constexpr int value = BBM_HIP_CT_WAVES; };   // A/B
#endif
// With VGroove's conditions straight-line (microfacet.hpp) the four unrolled pairs of k_eval_pdf_v4 are one basic
// block, and the scheduler, left to itself, interleaves them up to 106 VGPRs = 4 waves per SIMD (it was 91 = 5 with
// the body cut into nine blocks).  A floor of 5 waves makes it schedule for registers instead: 66 VGPRs, 7 waves,
// no scratch, in both the default and the exact-mode instantiation (-Rpass-analysis=kernel-resource-usage).  The
// floor is for that kernel only (eval_v4_waves): under it the world-space and per-lane kernels of
// Aggregate<Lambertian, CookTorrance> spilled 12-88 B per lane, so they and every other kernel keep eval_waves.
#ifndef BBM_HIP_CT_V4_WAVES
#define BBM_HIP_CT_V4_WAVES 5
#endif
template<> struct eval_v4_waves<CookTorranceM> { static constexpr int value = BBM_HIP_CT_V4_WAVES; };
using GGXM = Microfacet<GGX<false>, Uncorrelated, FresnelCook, Norm::Walter, true>;                        // bsdfmodel/ggx.h:27-33
using CookTorranceWalterM = Microfacet<Beckmann<false, true>, Uncorrelated, FresnelCook, Norm::Walter, true>;  // bsdfmodel/cooktorrancewalter.h:32-38

using CookTorranceHeitzM = Microfacet<Beckmann<true, true>, HeightCorrelated, FresnelCook, Norm::Walter, true>;   // bsdfmodel/cooktorranceheitz.h:33-39
using GGXHeitzM = Microfacet<GGX<true>, HeightCorrelated, FresnelCook, Norm::Walter, true>;                     // bsdfmodel/ggxheitz.h:28-34
// eval reads no glibc table (GGX's D, G1 and FresnelCook are rational / sqrt; Lambertian is a constant)
template<> struct uses_math_tables<Lambertian> { static constexpr bool value = false; };
template<> struct uses_math_tables<GGXM> { static constexpr bool value = false; };
template<> struct uses_math_tables<GGXHeitzM> { static constexpr bool value = false; };
using NganCookTorranceM = Microfacet<Beckmann<false, true>, VGroove, FresnelSchlick, Norm::Cook, true>;         // bsdfmodel/ngan.h:141-147
using PhongWalterM = Microfacet<PhongNdf, Uncorrelated, FresnelCook, Norm::Walter, true>;                         // bsdfmodel/phongwalter.h:27-33
#ifdef BBM_HIP_MIDTIER_WAVES   // A/B: the mid-tier microfacet variants' occupancy
template<> struct eval_waves<CookTorranceWalterM> { static constexpr int value = BBM_HIP_MIDTIER_WAVES; };
template<> struct eval_waves<CookTorranceHeitzM> { static constexpr int value = BBM_HIP_MIDTIER_WAVES; };
template<> struct eval_waves<PhongWalterM> { static constexpr int value = BBM_HIP_MIDTIER_WAVES; };
#endif
#ifdef BBM_HIP_MIDTIER_PIPE     // A/B: software-pipelined loop on a capped grid
template<> struct eval_pipeline<CookTorranceWalterM> { static constexpr bool value = true; };
template<> struct eval_pipeline<CookTorranceHeitzM> { static constexpr bool value = true; };
template<> struct eval_pipeline<PhongWalterM> { static constexpr bool value = true; };
template<> struct eval_grid_cap<CookTorranceWalterM> { static constexpr uint64_t value = BBM_HIP_MIDTIER_PIPE; };
template<> struct eval_grid_cap<CookTorranceHeitzM> { static constexpr uint64_t value = BBM_HIP_MIDTIER_PIPE; };
template<> struct eval_grid_cap<PhongWalterM> { static constexpr uint64_t value = BBM_HIP_MIDTIER_PIPE; };
#endif
#ifdef BBM_HIP_MIDTIER_NOPF     // A/B: their first-quad prefetch
template<> struct eval_prefetch<CookTorranceWalterM> { static constexpr bool value = false; };
template<> struct eval_prefetch<CookTorranceHeitzM> { static constexpr bool value = false; };
template<> struct eval_prefetch<PhongWalterM> { static constexpr bool value = false; };
#endif
using RibardiereM = Microfacet<StudentT<false>, Uncorrelated, FresnelCook, Norm::Walter, true>;                   // bsdfmodel/ribardiere.h:28-34
using RibardiereAnisoM = Microfacet<StudentT<true>, Uncorrelated, FresnelCook, Norm::Walter, true>;              // bsdfmodel/ribardiere.h:46-52

using LowMicrofacetM = Microfacet<LowNdf, VGroove, FresnelCook, Norm::Cook, true>;                             // bsdfmodel/lowmicrofacet.h:37-70, low.h:40-41
template<> struct eval_grid_cap<RibardiereM> { static constexpr uint64_t value = 2048; };
template<> struct eval_grid_cap<RibardiereAnisoM> { static constexpr uint64_t value = 2048; };
using WardM = Ward<0, true>;                  // bsdfmodel/ward.h:26-168
using WardDuerM = Ward<1, true>;              // bsdfmodel/wardduer.h:29-81
using WardDGMM = Ward<2, true>;               // bsdfmodel/wardduergeislermoroder.h:29-81
using NganWardM = Ward<0, false>;             // bsdfmodel/ngan.h:30-31
using NganWardDuerM = Ward<1, false>;         // bsdfmodel/ngan.h:37-38
using LafortuneM = Lafortune<true, false>;    // bsdfmodel/lafortune.h:28-172
using NganLafortuneM = Lafortune<false, true>;   // bsdfmodel/ngan.h:54-129
using ASM = AshikhminShirley<FresnelSchlickRGB, true, false, false>;                       // ashikhminshirley.h:29-221
using ASFullM = AshikhminShirley<FresnelSchlickRGB, true, false, true>;                    // ashikhminshirleyfull.h:31-191
using LowASM = AshikhminShirley<ScalarFresnel3<FresnelCook>, false, true, false>;          // bsdfmodel/low.h:24-25
using NganASM = AshikhminShirley<ScalarFresnel3<FresnelSchlick>, false, true, false>;      // bsdfmodel/ngan.h:157-158

// Aggregate(Lambertian, X): the form of every published fit (fits/*.fit), aggregatemodel.h:22-233
using AggBagherM = Aggregate<Lambertian, Bagher>;
using AggCookTorranceM = Aggregate<Lambertian, CookTorranceM>;
using AggGGXM = Aggregate<Lambertian, GGXM>;
template<> struct uses_math_tables<AggGGXM> { static constexpr bool value = false; };
using AggLowASM = Aggregate<Lambertian, LowASM>;
using AggLowMicrofacetM = Aggregate<Lambertian, LowMicrofacetM>;
using AggLowSmoothM = Aggregate<Lambertian, LowSmooth>;
using AggNganASM = Aggregate<Lambertian, NganASM>;
using AggPhongM = Aggregate<Lambertian, PhongLobe>;
using AggNganCookTorranceM = Aggregate<Lambertian, NganCookTorranceM>;
using AggNganLafortuneM = Aggregate<Lambertian, NganLafortuneM>;
using AggNganWardM = Aggregate<Lambertian, NganWardM>;
using AggNganWardDuerM = Aggregate<Lambertian, NganWardDuerM>;
using AggNganHeM = Aggregate<Lambertian, NganHeM>;    // fits/ngan_he.fit

// An aggregate's per-launch derived data is its children's (the He family's sampling CDF): B's block starts
// after A's parameters, and B's derived slots (B::kParams + ...) are then exactly the aggregate's own
// (A::kParams + B::kParams + ...), where B's device constructor (p + A::kParams) finds them.
template<class A, class B>
struct host_params<Aggregate<A, B>>
{
  static_assert(std::is_same_v<A, Lambertian>, "fused aggregates have a Lambertian first child");
  static int run(ParamBlock& p, uint32_t component, hipStream_t s, void** scratch)
  {
    ParamBlock q{};
    for (int k = A::kParams; k < kMaxParams; ++k) q.v[k - A::kParams] = p.v[k];
    if (const int rc = host_params<B>::run(q, component, s, scratch)) return rc;
    for (int k = A::kParams; k < kMaxParams; ++k) p.v[k] = q.v[k - A::kParams];
    return 0;
  }
  static void done(void* scratch, hipStream_t s) { host_params<B>::done(scratch, s); }
};

// sample_eval (sample_eval.hpp): the kernels whose quad form has scratch at check_waves' 128 VGPRs where the row's
// k_sample_v4 and k_eval_pdf_v4 have none; they run one lane per thread (bytes per lane in DESIGN.md §4.16).
// D: the default-mode kernel, E: the one the exact mode launches.
#define BBM_HIP_SAMPLE_EVAL_ONE_LANE_D(M) template<> struct sample_eval_quad<M, false> { static constexpr bool value = false; };
#define BBM_HIP_SAMPLE_EVAL_ONE_LANE_E(M) template<> struct sample_eval_quad<M, true> { static constexpr bool value = false; };
#define BBM_HIP_SAMPLE_EVAL_ONE_LANE(M) BBM_HIP_SAMPLE_EVAL_ONE_LANE_D(M) BBM_HIP_SAMPLE_EVAL_ONE_LANE_E(M)
BBM_HIP_SAMPLE_EVAL_ONE_LANE_E(CookTorranceM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE_E(NganCookTorranceM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(PhongWalterM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(RibardiereM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(RibardiereAnisoM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(LowMicrofacetM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(PhongLobe)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(LafortuneM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(NganLafortuneM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(ASM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(ASFullM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(LowASM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(NganASM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(Bagher)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggBagherM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggCookTorranceM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggLowASM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggLowMicrofacetM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggLowSmoothM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggNganASM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggPhongM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggNganCookTorranceM)
BBM_HIP_SAMPLE_EVAL_ONE_LANE(AggNganLafortuneM)
// tables: EPD's 8 B are left alone, its one-lane kernel has them too
template<> struct sample_eval_tab_quad<AggCookTorranceM, false> { static constexpr bool value = false; };
template<> struct sample_eval_tab_quad<LowMicrofacetM, true> { static constexpr bool value = false; };
template<> struct sample_eval_tab_quad<AggLowMicrofacetM, true> { static constexpr bool value = false; };
template<> struct sample_eval_tab_quad<AggNganCookTorranceM, false> { static constexpr bool value = false; };
template<> struct sample_eval_tab_quad<AggNganCookTorranceM, true> { static constexpr bool value = false; };

// The world-space kernels (FRAME), judged again on top of the above: a quad kernel that spills with
// the frames in registers -- to scratch, or to AGPRs at half the local kernel's waves (the He family, EPD's table
// kernel) -- where the row's one-lane world kernel does not.  U: the uniform call, T: the table call.
#define BBM_HIP_WORLD_ONE_LANE_UD(M) template<> struct sample_eval_world_quad<M, false> { static constexpr bool value = false; };
#define BBM_HIP_WORLD_ONE_LANE_UE(M) template<> struct sample_eval_world_quad<M, true> { static constexpr bool value = false; };
#define BBM_HIP_WORLD_ONE_LANE_TD(M) template<> struct sample_eval_tab_world_quad<M, false> { static constexpr bool value = false; };
#define BBM_HIP_WORLD_ONE_LANE_TE(M) template<> struct sample_eval_tab_world_quad<M, true> { static constexpr bool value = false; };
#define BBM_HIP_WORLD_ONE_LANE_U(M) BBM_HIP_WORLD_ONE_LANE_UD(M) BBM_HIP_WORLD_ONE_LANE_UE(M)
#define BBM_HIP_WORLD_ONE_LANE_T(M) BBM_HIP_WORLD_ONE_LANE_TD(M) BBM_HIP_WORLD_ONE_LANE_TE(M)
BBM_HIP_WORLD_ONE_LANE_U(HeM)
BBM_HIP_WORLD_ONE_LANE_U(HeWestinM)
BBM_HIP_WORLD_ONE_LANE_U(HeHolzschuchM)
BBM_HIP_WORLD_ONE_LANE_U(NganHeM)
BBM_HIP_WORLD_ONE_LANE_U(AggNganHeM)
BBM_HIP_WORLD_ONE_LANE_U(AggGGXM)
BBM_HIP_WORLD_ONE_LANE_U(AggNganWardM)
BBM_HIP_WORLD_ONE_LANE_U(AggNganWardDuerM)
BBM_HIP_WORLD_ONE_LANE_U(LowSmooth)
BBM_HIP_WORLD_ONE_LANE_U(Merl)
BBM_HIP_WORLD_ONE_LANE_UE(CookTorranceWalterM)
BBM_HIP_WORLD_ONE_LANE_UE(CookTorranceHeitzM)
BBM_HIP_WORLD_ONE_LANE_TE(CookTorranceM)
BBM_HIP_WORLD_ONE_LANE_TE(NganCookTorranceM)
BBM_HIP_WORLD_ONE_LANE_T(EpdM)
BBM_HIP_WORLD_ONE_LANE_T(Bagher)
BBM_HIP_WORLD_ONE_LANE_T(ASM)
BBM_HIP_WORLD_ONE_LANE_T(ASFullM)
BBM_HIP_WORLD_ONE_LANE_T(LowASM)
BBM_HIP_WORLD_ONE_LANE_T(NganASM)
BBM_HIP_WORLD_ONE_LANE_T(NganLafortuneM)
BBM_HIP_WORLD_ONE_LANE_T(AggBagherM)
BBM_HIP_WORLD_ONE_LANE_TE(AggCookTorranceM)
BBM_HIP_WORLD_ONE_LANE_T(AggGGXM)
BBM_HIP_WORLD_ONE_LANE_T(AggLowASM)
BBM_HIP_WORLD_ONE_LANE_TD(AggLowMicrofacetM)
BBM_HIP_WORLD_ONE_LANE_T(AggLowSmoothM)
BBM_HIP_WORLD_ONE_LANE_T(AggNganASM)
BBM_HIP_WORLD_ONE_LANE_T(AggPhongM)
BBM_HIP_WORLD_ONE_LANE_T(AggNganLafortuneM)


// eval_pdf in world space (eval_world.hpp, lanes.hpp over EvalTabWorldArgs), judged the same way.
// The frame is dead before the model runs, so no quad kernel gains scratch or AGPRs over its local form but the
// compact rows' eval + pdf quad (262-266 VGPRs + 6-10 AGPRs at one wave, the one-lane kernel 161-183 and none at two
// or three) -- a kernel the library launches only with compaction switched off (an experimental build); those rows
// have no world quad at all.  The table kernels need nothing: EPD's 8 B are in its one-lane kernel too.
template<class M, int MODE, bool EXACT> requires compact_eval<M>::value
struct eval_world_quad<M, MODE, EXACT> { static constexpr bool value = false; };

// The rows whose x and y roughness, sharpness or lobe coefficients run along the shading frame's X and Y: the
// tangent forms of the world-space calls exist for these alone.  For every other row -- the fused
// Aggregate<Lambertian, X> rows included, none of which has an anisotropic child -- value and pdf do not depend on
// the rotation about the normal, and a tangent call is the normal-only call.
template<class M> struct anisotropic { static constexpr bool value = false; };
#define BBM_HIP_ANISOTROPIC(M) template<> struct anisotropic<M> { static constexpr bool value = true; };
BBM_HIP_ANISOTROPIC(WardM)
BBM_HIP_ANISOTROPIC(WardDuerM)
BBM_HIP_ANISOTROPIC(WardDGMM)
BBM_HIP_ANISOTROPIC(CookTorranceHeitzM)
BBM_HIP_ANISOTROPIC(GGXHeitzM)
BBM_HIP_ANISOTROPIC(RibardiereAnisoM)
BBM_HIP_ANISOTROPIC(LafortuneM)
BBM_HIP_ANISOTROPIC(ASM)
BBM_HIP_ANISOTROPIC(ASFullM)

// The tangent kernels, judged on top of the world kernels' choice from the compiler's resource report (the table in
// DESIGN.md §4.20): a quad that spills with the tangent's twelve floats on top where its one-lane form does not runs
// one lane per thread.
// Two do (profiles/tangent_resources.txt): WardDuerGeislerMoroder's uniform quad (12 B) and RibardiereAnisotropic's
// exact-mode table quad (20 B); no eval_pdf quad gains scratch or AGPRs, the frame being dead before the model runs.
template<> struct sample_eval_tangent_quad<WardDGMM, false> { static constexpr bool value = false; };
template<> struct sample_eval_tab_tangent_quad<RibardiereAnisoM, true> { static constexpr bool value = false; };

}  // namespace bbmhip

// X(composition) per instantiation unit
#define BBM_HIP_MICROFACET_MODELS(X) \
  X(CookTorranceM) X(GGXM) X(CookTorranceWalterM) X(CookTorranceHeitzM) X(GGXHeitzM) X(NganCookTorranceM) \
  X(PhongWalterM) X(RibardiereM) X(RibardiereAnisoM) X(LowMicrofacetM)
#define BBM_HIP_LOBE_MODELS(X) \
  X(WardM) X(WardDuerM) X(WardDGMM) X(NganWardM) X(NganWardDuerM) X(PhongLobe) X(LafortuneM) X(NganLafortuneM) \
  X(ASM) X(ASFullM) X(LowASM) X(NganASM) X(LowSmooth)
#define BBM_HIP_DIFFUSE_MODELS(X) X(Lambertian) X(OrenNayar)
#define BBM_HIP_SPECTRAL_MODELS(X) X(Bagher)
#define BBM_HIP_EPD_MODELS(X) X(EpdM)
#define BBM_HIP_HE_MODELS(X) X(HeM) X(HeWestinM) X(HeHolzschuchM) X(NganHeM)
#define BBM_HIP_MERL_MODELS(X) X(Merl)
#define BBM_HIP_AGGREGATE_MODELS(X) \
  X(AggBagherM) X(AggCookTorranceM) X(AggGGXM) X(AggLowASM) X(AggLowMicrofacetM) X(AggLowSmoothM) X(AggNganASM) \
  X(AggPhongM) X(AggNganCookTorranceM) X(AggNganLafortuneM) X(AggNganWardM) X(AggNganWardDuerM) X(AggNganHeM)

// the anisotropic rows (anisotropic<M>), per unit: the tangent forms of the world-space calls
#define BBM_HIP_MICROFACET_TANGENT_MODELS(X) X(CookTorranceHeitzM) X(GGXHeitzM) X(RibardiereAnisoM)
#define BBM_HIP_LOBE_TANGENT_MODELS(X) X(WardM) X(WardDuerM) X(WardDGMM) X(LafortuneM) X(ASM) X(ASFullM)

#define BBM_HIP_INSTANTIATE(M)                                                   \
  template int launch_eval_pdf<M>(const EvalArgs&, int, hipStream_t);           \
  template int launch_sample<M>(const SampleArgs&, hipStream_t);                \
  template int launch_reflectance<M>(const ReflArgs&, hipStream_t);            \
  template int launch_loss<M>(const LossArgs&, hipStream_t);                  \
  template int launch_check<M>(int, const CheckArgs&, double*, hipStream_t);    \
  template int launch_image<M>(const ImageArgs&, hipStream_t);                \
  template int launch_eval_pdf_lanes<M, EvalVarArgs>(const EvalVarArgs&, int, hipStream_t);  \
  template int launch_sample_lanes<M, SampleVarArgs>(const SampleVarArgs&, hipStream_t);       \
  template int launch_reflectance_lanes<M, ReflVarArgs>(const ReflVarArgs&, hipStream_t);    \
  template int table_prepare<M>(const ParamBlock&, bool, hipStream_t, TableBlocks&); \
  template int launch_eval_pdf_lanes<M, EvalTabArgs>(const EvalTabArgs&, int, hipStream_t);  \
  template int launch_sample_lanes<M, SampleTabArgs>(const SampleTabArgs&, hipStream_t);       \
  template int launch_reflectance_lanes<M, ReflTabArgs>(const ReflTabArgs&, hipStream_t);    \
  template int launch_sample_eval<M>(const SampleEvalArgs&, hipStream_t);     \
  template int launch_sample_eval_tab<M>(const SampleEvalTabArgs&, hipStream_t); \
  template int launch_sample_eval_world<M>(const SampleEvalArgs&, hipStream_t); \
  template int launch_sample_eval_tab_world<M>(const SampleEvalTabArgs&, hipStream_t); \
  template int launch_eval_pdf_world<M>(const EvalWorldArgs&, int, hipStream_t); \
  template int launch_eval_pdf_tab_world<M>(const EvalTabWorldArgs&, int, hipStream_t);
#define BBM_HIP_EXTERN(M)                                                       \
  extern template int launch_eval_pdf<M>(const EvalArgs&, int, hipStream_t);    \
  extern template int launch_sample<M>(const SampleArgs&, hipStream_t);         \
  extern template int launch_reflectance<M>(const ReflArgs&, hipStream_t);     \
  extern template int launch_loss<M>(const LossArgs&, hipStream_t);           \
  extern template int launch_check<M>(int, const CheckArgs&, double*, hipStream_t); \
  extern template int launch_image<M>(const ImageArgs&, hipStream_t);         \
  extern template int launch_eval_pdf_lanes<M, EvalVarArgs>(const EvalVarArgs&, int, hipStream_t); \
  extern template int launch_sample_lanes<M, SampleVarArgs>(const SampleVarArgs&, hipStream_t); \
  extern template int launch_reflectance_lanes<M, ReflVarArgs>(const ReflVarArgs&, hipStream_t); \
  extern template int table_prepare<M>(const ParamBlock&, bool, hipStream_t, TableBlocks&); \
  extern template int launch_eval_pdf_lanes<M, EvalTabArgs>(const EvalTabArgs&, int, hipStream_t); \
  extern template int launch_sample_lanes<M, SampleTabArgs>(const SampleTabArgs&, hipStream_t); \
  extern template int launch_reflectance_lanes<M, ReflTabArgs>(const ReflTabArgs&, hipStream_t); \
  extern template int launch_sample_eval<M>(const SampleEvalArgs&, hipStream_t); \
  extern template int launch_sample_eval_tab<M>(const SampleEvalTabArgs&, hipStream_t); \
  extern template int launch_sample_eval_world<M>(const SampleEvalArgs&, hipStream_t); \
  extern template int launch_sample_eval_tab_world<M>(const SampleEvalTabArgs&, hipStream_t); \
  extern template int launch_eval_pdf_world<M>(const EvalWorldArgs&, int, hipStream_t); \
  extern template int launch_eval_pdf_tab_world<M>(const EvalTabWorldArgs&, int, hipStream_t);
#define BBM_HIP_INSTANTIATE_TANGENT(M)                                         \
  static_assert(anisotropic<M>::value, "tangent kernels are for the anisotropic rows"); \
  template int launch_sample_eval_tangent<M>(const SampleEvalTangentArgs&, hipStream_t); \
  template int launch_sample_eval_tab_tangent<M>(const SampleEvalTabTangentArgs&, hipStream_t); \
  template int launch_eval_pdf_tangent<M>(const EvalTangentArgs&, int, hipStream_t); \
  template int launch_eval_pdf_tab_tangent<M>(const EvalTabTangentArgs&, int, hipStream_t);
#define BBM_HIP_EXTERN_TANGENT(M)                                              \
  extern template int launch_sample_eval_tangent<M>(const SampleEvalTangentArgs&, hipStream_t); \
  extern template int launch_sample_eval_tab_tangent<M>(const SampleEvalTabTangentArgs&, hipStream_t); \
  extern template int launch_eval_pdf_tangent<M>(const EvalTangentArgs&, int, hipStream_t); \
  extern template int launch_eval_pdf_tab_tangent<M>(const EvalTabTangentArgs&, int, hipStream_t);
