// bbm_amd/csrc/host.hpp -- what the host side of every unit shares: the error record, the launch check, the grid
// size of a grid-stride launch and the stream-ordered scratch pool.  No device code and no model knowledge.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace bbmhip {

// Record `msg` as the calling thread's last error (bbm_hip_last_error) and return `code` (bbm_hip.hip).
int fail(int code, const std::string& msg);

// After a kernel launch: BBM_HIP_OK, or BBM_HIP_ERR_HIP with "<what>: <HIP's error string>" as the last error
// (`what` defaults to "kernel launch failed").
int launched(const char* what = nullptr);

// Workgroups of `block` threads that cover n items, at most `max_blocks` (grid-stride kernels take the rest)
inline unsigned grid_blocks(uint64_t n, unsigned block, uint64_t max_blocks)
{
  const uint64_t b = (n + block - 1) / block;
  return unsigned(b > max_blocks ? max_blocks : b);
}

// Stream-ordered device scratch (scratch.hip): per-launch derived data (the tabulated samplers' CDFs) and the
// composed aggregates' per-lane temporaries.  A released block keeps an event recorded on the releasing
// stream; re-acquiring it on the same stream needs nothing (stream order), on another stream that stream
// waits for the event on the GPU.  No host synchronisation; blocks are kept for reuse.  (Replaces
// hipMallocAsync / hipFreeAsync on the caller's stream, under which tests/cpp/adapter_check -- a plain C++
// host program on the null stream -- saw He CDFs and composed-aggregate outputs corrupted at random.)
void* scratch_acquire(size_t bytes, hipStream_t s);
std::string scratch_failure();   // why the calling thread's last scratch_acquire returned nullptr
void scratch_release(void* p, hipStream_t s);

}  // namespace bbmhip
