// bbm_amd/csrc/scratch.hip -- the stream-ordered device scratch pool (host.hpp) and its bbm_hip_scratch_* entry
// points.  Host code only.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bbm_hip.h"
#include "host.hpp"

namespace bbmhip {

// ------------------------------------------------------------------------ stream-ordered scratch

namespace {
struct ScratchBlock
{
  void* p;
  size_t bytes;
  int device;
  hipEvent_t released;     // recorded on `last` when the block was released
  hipStream_t last;
  bool busy, used;
  bool pinned;             // handed out while `last` was capturing a graph: the graph keeps the address, so the
                           // block is never handed out or freed again (bbm_hip_scratch_trim_captured aside)
};
std::mutex g_scratch_mu;
std::vector<ScratchBlock> g_scratch;
}  // namespace

namespace {
// idle bytes kept for reuse before released blocks are returned to the device (BBM_HIP_SCRATCH_RETAIN_MB)
size_t retain_limit()
{
  static const size_t v = [] {
    const char* e = std::getenv("BBM_HIP_SCRATCH_RETAIN_MB");
    return size_t(e ? std::strtoull(e, nullptr, 10) : 1024ull) << 20;
  }();
  return v;
}

// frees idle blocks (caller holds the lock): wait = false only those whose last use has completed on the GPU;
// wait = true all of them, after their release event.  `keep`: idle bytes that may stay.  Returns bytes freed.
size_t free_idle(bool wait, size_t keep)
{
  size_t idle = 0, freed = 0;
  for (const ScratchBlock& b : g_scratch) idle += b.busy ? 0 : b.bytes;
  for (size_t i = g_scratch.size(); i-- > 0 && idle > keep;)
  {
    ScratchBlock& b = g_scratch[i];
    if (b.busy || b.pinned) continue;
    if (b.used && (wait ? hipEventSynchronize(b.released) : hipEventQuery(b.released)) != hipSuccess) continue;
    (void)hipFree(b.p);
    (void)hipEventDestroy(b.released);
    idle -= b.bytes;
    freed += b.bytes;
    g_scratch.erase(g_scratch.begin() + long(i));
  }
  return freed;
}
}  // namespace

thread_local std::string g_scratch_why;

std::string scratch_failure() { return g_scratch_why.empty() ? std::string("out of device memory") : g_scratch_why; }

void* scratch_acquire(size_t bytes, hipStream_t s)
{
  g_scratch_why.clear();
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  bytes = (bytes + 255) & ~size_t(255);
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (const hipError_t e = hipStreamIsCapturing(s, &cap); e != hipSuccess)
  {
    // e.g. the legacy null stream while another stream is under a global-mode capture
    g_scratch_why = std::string("the stream's capture status cannot be read (hipStreamIsCapturing: ") +
                    hipGetErrorString(e) + "; a call on the null stream during a global-mode capture?)";
    return nullptr;
  }
  if (cap != hipStreamCaptureStatusNone)
  {
    // graph capture: a fresh block that belongs to the graph from now on.  No idle block is reused (its release
    // event was recorded outside the capture, and waiting on it would tie the graph to a pre-capture event), and
    // the allocation runs in relaxed capture mode (hipMalloc is not allowed under a global-mode capture).
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    ScratchBlock b{nullptr, bytes, dev, nullptr, s, true, true, true};
    const bool ok = hipMalloc(&b.p, bytes) == hipSuccess;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (!ok) return nullptr;
    g_scratch.push_back(b);
    return b.p;
  }
  // best fit among idle blocks of this device, but not one much larger than the request (a 360-byte CDF must not
  // pin a block sized for 125M lanes)
  ScratchBlock* best = nullptr;
  for (ScratchBlock& b : g_scratch)
    if (!b.busy && !b.pinned && b.device == dev && b.bytes >= bytes && (b.bytes <= 4 * bytes || b.bytes - bytes <= (size_t(1) << 20)) &&
        (!best || b.bytes < best->bytes))
      best = &b;
  if (best)
  {
    // its last user's work must be done before this stream writes it: free on the same stream (stream
    // order), otherwise a GPU-side wait on the release event
    if (best->used && best->last != s && hipStreamWaitEvent(s, best->released, 0) != hipSuccess) return nullptr;
    best->busy = true;
    return best->p;
  }
  ScratchBlock b{nullptr, bytes, dev, nullptr, s, true, false, false};
  if (hipMalloc(&b.p, bytes) != hipSuccess)
  {
    // out of device memory: return every idle block (after its last use) and try once more
    (void)hipGetLastError();
    free_idle(true, 0);
    if (hipMalloc(&b.p, bytes) != hipSuccess) return nullptr;
  }
  if (hipEventCreateWithFlags(&b.released, hipEventDisableTiming) != hipSuccess)
  {
    (void)hipFree(b.p);
    return nullptr;
  }
  g_scratch.push_back(b);
  return b.p;
}

void scratch_release(void* p, hipStream_t s)
{
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  for (ScratchBlock& b : g_scratch)
    if (b.p == p)
    {
      if (b.pinned) return;      // the captured graph owns it: no event, no reuse, and no freeing inside a capture
      (void)hipEventRecord(b.released, s);
      b.last = s;
      b.busy = false;
      b.used = true;
      break;
    }
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) free_idle(false, retain_limit());
}

size_t scratch_trim()
{
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  return free_idle(true, 0);
}

size_t scratch_trim_captured()
{
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  size_t freed = 0;
  bool synced = false;
  for (size_t i = g_scratch.size(); i-- > 0;)
  {
    ScratchBlock& b = g_scratch[i];
    if (!b.pinned) continue;
    if (!synced)
    {
      (void)hipDeviceSynchronize();
      synced = true;
    }
    (void)hipFree(b.p);
    if (b.released) (void)hipEventDestroy(b.released);
    freed += b.bytes;
    g_scratch.erase(g_scratch.begin() + long(i));
  }
  return freed + free_idle(true, 0);
}

size_t scratch_bytes()
{
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  size_t t = 0;
  for (const ScratchBlock& b : g_scratch) t += b.bytes;
  return t;
}

}  // namespace bbmhip

using namespace bbmhip;

extern "C" {

size_t bbm_hip_scratch_trim(void) { return scratch_trim(); }

size_t bbm_hip_scratch_trim_captured(void) { return scratch_trim_captured(); }

size_t bbm_hip_scratch_bytes(void) { return scratch_bytes(); }

}  // extern "C"
