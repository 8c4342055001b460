// bbm_amd/csrc/set.hpp -- material sets: the model-independent kernels that carry a batch whose
// lanes belong to different material tables to the table kernels and back.  A plan is the stable partition of the
// lanes by table ("row"): k_set_count, k_set_scan and k_set_place build it; k_set_gather moves the input streams into
// per-row segments and k_set_scatter puts the results back.  The kernels are in set.hip; the entry points
// (bbm_hip_set_*) are in bbm_hip.hip, which calls the table entry points on the segments: one check function and one
// row loop per call kind (set_eval_pdf_check / _rows, set_sample_eval_check / _rows).  A call in plan order is that
// loop on the caller's streams; a call in lane order (set_lane_order) is the same loop between a gather into scratch
// and a scatter out of it, the scratch sized by the streams it entered into the two moves.  No model knowledge.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bbmhip {

constexpr uint32_t kSetMaxRows = 32;                  // tables in one set
constexpr uint32_t kSetBlock = 256;                   // threads of every set kernel
constexpr uint32_t kSetPasses = 16;                   // 256-lane passes one workgroup ranks
constexpr uint32_t kSetTile = kSetBlock * kSetPasses; // lanes a workgroup counts and ranks: 4096
constexpr uint32_t kSetScanPer = 4;                   // entries per thread in one pass of the scan loop
constexpr uint32_t kSetScanChunk = kSetBlock * kSetScanPer;   // entries one pass of the scan loop covers: 1024
constexpr uint32_t kSetNone = 0xFFFFFFFFu;            // src of a padding slot; the index of a masked-index lane
constexpr int kSetMaxIn = 9;                          // float streams a call gathers (normal, in, out / normal, out, xi)
constexpr int kSetMaxOut = 11;                        // four-byte streams a call scatters (dir, pdf, flag, value, weight)

// The rows of a set as the kernels see them, by value in the kernarg: row k owns the global ids
// [off[k], off[k + 1]); off[rows] is the total.
struct SetRows
{
  uint32_t rows;
  uint32_t off[kSetMaxRows + 1];
};

// What k_set_scan leaves for k_set_place and for the host, in device memory (uint32 each):
//   seg[0 .. rows]   first slot of each row's segment, a multiple of four; seg[rows] is the capacity
//   end[0 .. rows)   one past the row's last lane: the slots [end[k], seg[k + 1]) are padding
//   delta[0 .. rows) what turns the flat exclusive sum of a (row, workgroup) entry into its first slot (mod 2^32)
struct SetMeta
{
  uint32_t seg[kSetMaxRows + 1];
  uint32_t end[kSetMaxRows];
  uint32_t delta[kSetMaxRows];
};

struct SetPlanArgs
{
  SetRows rows;
  const uint32_t* material;    // n global ids
  uint32_t n;
  uint32_t groups;             // workgroups of k_set_count / k_set_place: ceil(n / kSetTile)
  uint32_t* counts;            // rows x groups, row-major: counts, then (k_set_scan) their flat exclusive sums
  SetMeta* meta;
  uint32_t* src;               // slots
  uint32_t* local;             // slots
  uint32_t slots;              // allocated slots of src and local: every computed slot is compared against it
  uint32_t drop;               // a compact plan: a lane whose id is past the total is in no slot (else row 0's)
};

// One gather or scatter: `count` (at most kSetMaxOut) four-byte streams between caller arrays of n lanes (4-byte
// aligned) and sorted arrays of `capacity` slots (16-byte aligned, capacity a multiple of four).
struct SetMoveArgs
{
  const uint32_t* src;         // capacity slots
  uint32_t n, capacity;
  int count;
  const uint32_t* from[kSetMaxOut];
  uint32_t* to[kSetMaxOut];
  const uint8_t* mask_from;    // gather only: n bytes, or nullptr
  uint8_t* mask_to;            // capacity bytes (4-byte aligned)
};

// Enqueue the three plan kernels on s.  counts: rows x groups uint32 of scratch.
int set_plan_launch(const SetPlanArgs& a, hipStream_t s);
// Enqueue one gather (lane -> slot; padding slots get zeros and mask 0) or scatter (slot -> lane).
int set_gather_launch(const SetMoveArgs& a, hipStream_t s);
int set_scatter_launch(const SetMoveArgs& a, hipStream_t s);
// The gather in its other shape, for measurement: every load of a thread is issued before its
// first store.  Same arguments, same result.
int set_gather_launch_batched(const SetMoveArgs& a, hipStream_t s);

}  // namespace bbmhip
