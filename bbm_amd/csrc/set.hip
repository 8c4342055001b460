// bbm_amd/csrc/set.hip -- the kernels of material sets (set.hpp).  Model-independent.
//
// The plan is a stable counting sort of the lanes by row in three launches, with no atomics on global memory and no
// workgroup waiting for another: k_set_count (a histogram per workgroup), k_set_scan (one workgroup: the flat
// exclusive sum of the rows x workgroups counts, and the segment starts rounded up to four), k_set_place (the same
// rows again, ranked per wave with ballots, the wave totals combined through LDS).  k_set_gather / k_set_scatter move
// four slots per thread: 16-byte accesses on the sorted side, 4-byte gathers or scatters on the caller's side.
// k_set_count<true> / k_set_place<true> build the compact plan (§4.21): a lane whose id is out of range is in no slot.
// Every index read from device memory is compared against its bound before it is used: src[j] against n, a computed
// slot against the allocated slots.
#include "set.hpp"

#include "../../include/bbm_hip.h"
#include "host.hpp"
#include "math.hpp"   // math_tables_init(): the prologue every kernel of the library runs

namespace bbmhip {

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kWaves = kSetBlock / 64;
static_assert(kSetBlock == 256 && kWaves == 4 && kSetMaxRows == 32, "the LDS layouts below are written for these");

// The row that owns the global id g and g's index in that row's table; an id past the total (a negative int32
// included) is row 0's masked-index lane, or (DROP, a compact plan) no lane at all: `valid` is cleared and the lane
// takes part in no ballot.  rows.off sits in SGPRs: a short scalar compare loop.
template<bool DROP>
__device__ __forceinline__ uint32_t row_of(const SetRows& rows, uint32_t g, uint32_t& local, bool& valid)
{
  uint32_t r = 0, first = 0;
  for (uint32_t k = 1; k < rows.rows; ++k)
    if (g >= rows.off[k])
    {
      r = k;
      first = rows.off[k];
    }
  const bool in_range = g < rows.off[rows.rows];
  if constexpr (DROP) valid = valid && in_range;
  local = in_range ? g - first : kSetNone;
  return in_range ? r : 0u;
}

// One wave: the number of valid lanes below this one with the same row.  per_row(r, count) runs on one lane for every
// row present.  Wave-uniform control flow: one round of two ballots per row present.
template<class F>
__device__ __forceinline__ uint32_t wave_rank(bool valid, uint32_t row, F&& per_row)
{
  const uint32_t lane = __lane_id();
  uint32_t rank = 0;
  bool pending = valid;
  for (;;)
  {
    const unsigned long long todo = __ballot(pending);
    if (todo == 0) break;
    const int leader = __ffsll(todo) - 1;
    const uint32_t r = uint32_t(__shfl(int(row), leader));
    const bool mine = pending && row == r;
    const unsigned long long m = __ballot(mine);
    if (mine)
    {
      rank = uint32_t(__popcll(m & ((1ull << lane) - 1ull)));
      pending = false;
    }
    if (int(lane) == leader) per_row(r, uint32_t(__popcll(m)));
  }
  return rank;
}

// the 256-lane passes of workgroup `group` that hold a lane
__device__ __forceinline__ uint32_t passes_of(uint32_t n, uint32_t group)
{
  const uint64_t first = uint64_t(group) * kSetTile;
  if (first >= n) return 0;
  const uint64_t left = (uint64_t(n) - first + kSetBlock - 1) / kSetBlock;
  return left < kSetPasses ? uint32_t(left) : kSetPasses;
}

template<bool DROP>
__global__ __launch_bounds__(kSetBlock) void k_set_count(SetPlanArgs a)
{
  math_tables_init();
  __shared__ uint32_t hist[kSetMaxRows];
  const uint32_t tid = threadIdx.x;
  if (tid < kSetMaxRows) hist[tid] = 0;
  __syncthreads();
  const uint32_t passes = passes_of(a.n, blockIdx.x);
  for (uint32_t p = 0; p < passes; ++p)
  {
    const uint64_t i = uint64_t(blockIdx.x) * kSetTile + p * kSetBlock + tid;
    bool valid = i < a.n;
    uint32_t local;
    const uint32_t row = valid ? row_of<DROP>(a.rows, __builtin_nontemporal_load(a.material + i), local, valid) : 0u;
    wave_rank(valid, row, [&](uint32_t r, uint32_t c) { atomicAdd(&hist[r], c); });
  }
  __syncthreads();
  if (tid < a.rows.rows && blockIdx.x < a.groups) a.counts[uint64_t(tid) * a.groups + blockIdx.x] = hist[tid];
}

// One workgroup.  The flat exclusive sum over counts (row-major, kSetScanChunk entries per pass of the loop) replaces
// the counts; the sum at each row's first entry gives the row totals, from which one thread lays the segments out.
__global__ __launch_bounds__(kSetBlock) void k_set_scan(SetPlanArgs a)
{
  math_tables_init();
  __shared__ uint32_t wave_total[kWaves];
  __shared__ uint32_t row_first[kSetMaxRows];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t total = a.rows.rows * a.groups;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < total; base += kSetScanChunk)
  {
    const uint32_t e0 = base + tid * kSetScanPer;
    uint32_t v[kSetScanPer], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSetScanPer; ++j)
    {
      v[j] = (e0 + j < total) ? a.counts[e0 + j] : 0u;
      sum += v[j];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
      const uint32_t up = uint32_t(__shfl_up(int(incl), d));
      if (int(lane) >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, chunk = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w)
    {
      const uint32_t t = wave_total[w];
      before += w < wave ? t : 0u;
      chunk += t;
    }
    uint32_t excl = carry + before + (incl - sum);
#pragma unroll
    for (uint32_t j = 0; j < kSetScanPer; ++j)
    {
      const uint32_t e = e0 + j;
      if (e < total)
      {
        if (e % a.groups == 0) row_first[e / a.groups] = excl;
        a.counts[e] = excl;
        excl += v[j];
      }
    }
    carry += chunk;
    __syncthreads();
  }
  if (tid == 0)
  {
    uint32_t pos = 0;
    for (uint32_t k = 0; k < a.rows.rows; ++k)
    {
      const uint32_t count = (k + 1 < a.rows.rows ? row_first[k + 1] : carry) - row_first[k];
      a.meta->seg[k] = pos;
      a.meta->end[k] = pos + count;
      a.meta->delta[k] = pos - row_first[k];
      pos = (pos + count + 3u) & ~3u;
    }
    a.meta->seg[a.rows.rows] = pos;
  }
}

template<bool DROP>
__global__ __launch_bounds__(kSetBlock) void k_set_place(SetPlanArgs a)
{
  math_tables_init();
  __shared__ uint32_t run[kSetMaxRows];             // the next free slot of each row for this workgroup
  __shared__ uint32_t wave_count[kWaves][kSetMaxRows];
  const uint32_t tid = threadIdx.x, wave = tid >> 6;
  if (tid < kSetMaxRows)
  {
    run[tid] = tid < a.rows.rows ? a.counts[uint64_t(tid) * a.groups + blockIdx.x] + a.meta->delta[tid] : 0u;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) wave_count[w][tid] = 0;
  }
  const uint32_t passes = passes_of(a.n, blockIdx.x);
  for (uint32_t p = 0; p < passes; ++p)
  {
    __syncthreads();
    const uint64_t i = uint64_t(blockIdx.x) * kSetTile + p * kSetBlock + tid;
    bool valid = i < a.n;
    uint32_t local = kSetNone;
    const uint32_t row = valid ? row_of<DROP>(a.rows, __builtin_nontemporal_load(a.material + i), local, valid) : 0u;
    const uint32_t rank = wave_rank(valid, row, [&](uint32_t r, uint32_t c) { wave_count[wave][r] = c; });
    __syncthreads();
    if (valid)
    {
      uint32_t slot = run[row] + rank;
#pragma unroll
      for (uint32_t w = 0; w < kWaves; ++w) slot += w < wave ? wave_count[w][row] : 0u;
      if (slot < a.slots)
      {
        a.src[slot] = uint32_t(i);
        a.local[slot] = local;
      }
    }
    __syncthreads();
    if (tid < kSetMaxRows)
    {
      uint32_t sum = 0;
#pragma unroll
      for (uint32_t w = 0; w < kWaves; ++w)
      {
        sum += wave_count[w][tid];
        wave_count[w][tid] = 0;
      }
      run[tid] += sum;
    }
  }
  // the padding slots after each row's lanes
  if (blockIdx.x == 0 && tid < a.rows.rows)
  {
    const uint32_t end = a.meta->end[tid], next = a.meta->seg[tid + 1];
    for (uint32_t slot = end; slot < next && slot - end < 4u; ++slot)
      if (slot < a.slots)
      {
        a.src[slot] = kSetNone;
        a.local[slot] = kSetNone;
      }
  }
}

__global__ __launch_bounds__(kSetBlock) void k_set_gather(SetMoveArgs a)
{
  math_tables_init();
  const uint32_t q = blockIdx.x * kSetBlock + threadIdx.x;
  if (q >= (a.capacity >> 2)) return;
  const u4 sv = reinterpret_cast<const u4*>(a.src)[q];
  const uint32_t s[4] = {sv.x, sv.y, sv.z, sv.w};
  const bool ok[4] = {s[0] < a.n, s[1] < a.n, s[2] < a.n, s[3] < a.n};
#pragma unroll
  for (int c = 0; c < kSetMaxIn; ++c)
    if (c < a.count)
    {
      uint32_t v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ok[j] ? __builtin_nontemporal_load(a.from[c] + s[j]) : 0u;
      __builtin_nontemporal_store(u4{v[0], v[1], v[2], v[3]}, reinterpret_cast<u4*>(a.to[c]) + q);
    }
  if (a.mask_to)
  {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const uint32_t byte = ok[j] ? (a.mask_from ? uint32_t(a.mask_from[s[j]]) : 1u) : 0u;
      m |= byte << (8 * j);
    }
    reinterpret_cast<uint32_t*>(a.mask_to)[q] = m;
  }
}

// k_set_gather with every load of the thread (count x 4 values, the mask bytes included) issued before its first
// store: up to 36 values in flight per thread against four.
__global__ __launch_bounds__(kSetBlock) void k_set_gather_batched(SetMoveArgs a)
{
  math_tables_init();
  const uint32_t q = blockIdx.x * kSetBlock + threadIdx.x;
  if (q >= (a.capacity >> 2)) return;
  const u4 sv = reinterpret_cast<const u4*>(a.src)[q];
  const uint32_t s[4] = {sv.x, sv.y, sv.z, sv.w};
  const bool ok[4] = {s[0] < a.n, s[1] < a.n, s[2] < a.n, s[3] < a.n};
  uint32_t v[kSetMaxIn][4];
#pragma unroll
  for (int c = 0; c < kSetMaxIn; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      v[c][j] = (c < a.count && ok[j]) ? __builtin_nontemporal_load(a.from[c] + s[j]) : 0u;
  uint32_t m = 0;
  if (a.mask_to)
  {
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const uint32_t byte = ok[j] ? (a.mask_from ? uint32_t(a.mask_from[s[j]]) : 1u) : 0u;
      m |= byte << (8 * j);
    }
  }
#pragma unroll
  for (int c = 0; c < kSetMaxIn; ++c)
    if (c < a.count)
      __builtin_nontemporal_store(u4{v[c][0], v[c][1], v[c][2], v[c][3]}, reinterpret_cast<u4*>(a.to[c]) + q);
  if (a.mask_to) reinterpret_cast<uint32_t*>(a.mask_to)[q] = m;
}

__global__ __launch_bounds__(kSetBlock) void k_set_scatter(SetMoveArgs a)
{
  math_tables_init();
  const uint32_t q = blockIdx.x * kSetBlock + threadIdx.x;
  if (q >= (a.capacity >> 2)) return;
  const u4 sv = reinterpret_cast<const u4*>(a.src)[q];
  const uint32_t s[4] = {sv.x, sv.y, sv.z, sv.w};
  const bool ok[4] = {s[0] < a.n, s[1] < a.n, s[2] < a.n, s[3] < a.n};
#pragma unroll
  for (int c = 0; c < kSetMaxOut; ++c)
    if (c < a.count)
    {
      const u4 vv = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a.from[c]) + q);
      const uint32_t v[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ok[j]) __builtin_nontemporal_store(v[j], a.to[c] + s[j]);
    }
}

int set_launched(const char* what)
{
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(BBM_HIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(err));
  return BBM_HIP_OK;
}

}  // namespace

int set_plan_launch(const SetPlanArgs& a, hipStream_t s)
{
  if (a.drop)
    hipLaunchKernelGGL(k_set_count<true>, dim3(a.groups), dim3(kSetBlock), 0, s, a);
  else
    hipLaunchKernelGGL(k_set_count<false>, dim3(a.groups), dim3(kSetBlock), 0, s, a);
  hipLaunchKernelGGL(k_set_scan, dim3(1), dim3(kSetBlock), 0, s, a);
  if (a.drop)
    hipLaunchKernelGGL(k_set_place<true>, dim3(a.groups), dim3(kSetBlock), 0, s, a);
  else
    hipLaunchKernelGGL(k_set_place<false>, dim3(a.groups), dim3(kSetBlock), 0, s, a);
  return set_launched("material plan launch failed");
}

int set_gather_launch(const SetMoveArgs& a, hipStream_t s)
{
  const unsigned blocks = grid_blocks(a.capacity >> 2, kSetBlock, 0x7fffffffull);
  hipLaunchKernelGGL(k_set_gather, dim3(blocks), dim3(kSetBlock), 0, s, a);
  return set_launched("material set gather launch failed");
}

int set_gather_launch_batched(const SetMoveArgs& a, hipStream_t s)
{
  const unsigned blocks = grid_blocks(a.capacity >> 2, kSetBlock, 0x7fffffffull);
  hipLaunchKernelGGL(k_set_gather_batched, dim3(blocks), dim3(kSetBlock), 0, s, a);
  return set_launched("material set gather launch failed");
}

int set_scatter_launch(const SetMoveArgs& a, hipStream_t s)
{
  const unsigned blocks = grid_blocks(a.capacity >> 2, kSetBlock, 0x7fffffffull);
  hipLaunchKernelGGL(k_set_scatter, dim3(blocks), dim3(kSetBlock), 0, s, a);
  return set_launched("material set scatter launch failed");
}

}  // namespace bbmhip
