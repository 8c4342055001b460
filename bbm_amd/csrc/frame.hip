// bbm_amd/csrc/frame.hip -- bbm_hip_frame_to_local / bbm_hip_frame_to_global: a batch of vectors into or out of the
// shading frame of one normal per lane (frame.hpp), and their tangent forms
// bbm_hip_frame_to_local_tangent / _to_global_tangent (A = FrameTangentArgs: the frame of a normal and a tangent per
// lane, §4.20).  Model-independent: one quad and one one-lane kernel per direction and form.  36 B per lane (48 with
// the tangent) and a few dozen VALU: bound by HBM.
#include "kernels.hpp"

namespace bbmhip {

namespace {

// Four lanes per thread: six 16-byte nontemporal loads and three 16-byte nontemporal stores; every array 16-byte
// aligned and the mask 4-byte aligned (checked on the host).  A full grid; the n % 4 tail runs scalar in block 0.
template<class A> constexpr bool frame_tangent = std::is_same_v<A, FrameTangentArgs>;

// lane i's tangent, read only by the tangent form
template<class A>
__device__ __forceinline__ v3 tangent_at(const A& a, uint64_t i)
{
  if constexpr (frame_tangent<A>) return mk3(a.tx[i], a.ty[i], a.tz[i]);
  else return mk3(0.0f, 0.0f, 0.0f);
}

template<bool TO_LOCAL, class A>
__global__ __launch_bounds__(kBlock) void k_frame_v4(A a)
{
  constexpr bool TAN = frame_tangent<A>;
  math_tables_init();
  const uint64_t n4 = a.n >> 2;
  const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t < n4)
  {
    const float4 nx = ld4<true>(a.nx, t), ny = ld4<true>(a.ny, t), nz = ld4<true>(a.nz, t);
    const float4 x = ld4<true>(a.x, t), y = ld4<true>(a.y, t), z = ld4<true>(a.z, t);
    float4 tx = {}, ty = {}, tz = {};
    if constexpr (TAN) { tx = ld4<true>(a.tx, t); ty = ld4<true>(a.ty, t); tz = ld4<true>(a.tz, t); }
    const float ttx[4] = {tx.x, tx.y, tx.z, tx.w}, tty[4] = {ty.x, ty.y, ty.z, ty.w}, ttz[4] = {tz.x, tz.y, tz.z, tz.w};
    const uint32_t mk = a.mask ? reinterpret_cast<const uint32_t*>(a.mask)[t] : 0x01010101u;
    const float nnx[4] = {nx.x, nx.y, nx.z, nx.w}, nny[4] = {ny.x, ny.y, ny.z, ny.w}, nnz[4] = {nz.x, nz.y, nz.z, nz.w};
    const float vx[4] = {x.x, x.y, x.z, x.w}, vy[4] = {y.x, y.y, y.z, y.w}, vz[4] = {z.x, z.y, z.z, z.w};
    v3 r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      r[j] = frame_apply<TO_LOCAL, TAN>(mk3(nnx[j], nny[j], nnz[j]), mk3(vx[j], vy[j], vz[j]),
                                        ((mk >> (8 * j)) & 0xffu) != 0, mk3(ttx[j], tty[j], ttz[j]));
    st4<true>(a.rx, t, r[0].x, r[1].x, r[2].x, r[3].x);
    st4<true>(a.ry, t, r[0].y, r[1].y, r[2].y, r[3].y);
    st4<true>(a.rz, t, r[0].z, r[1].z, r[2].z, r[3].z);
  }
  if (blockIdx.x == 0 && threadIdx.x < (a.n & 3))
  {
    const uint64_t i = (n4 << 2) + threadIdx.x;
    const v3 r = frame_apply<TO_LOCAL, TAN>(mk3(a.nx[i], a.ny[i], a.nz[i]), mk3(a.x[i], a.y[i], a.z[i]),
                                            a.mask ? (a.mask[i] != 0) : true, tangent_at(a, i));
    a.rx[i] = r.x; a.ry[i] = r.y; a.rz[i] = r.z;
  }
}

// One lane per thread: unaligned arrays.
template<bool TO_LOCAL, class A>
__global__ __launch_bounds__(kBlock) void k_frame_v1(A a)
{
  constexpr bool TAN = frame_tangent<A>;
  math_tables_init();
  const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const v3 r = frame_apply<TO_LOCAL, TAN>(mk3(a.nx[i], a.ny[i], a.nz[i]), mk3(a.x[i], a.y[i], a.z[i]),
                                          a.mask ? (a.mask[i] != 0) : true, tangent_at(a, i));
  a.rx[i] = r.x; a.ry[i] = r.y; a.rz[i] = r.z;
}

template<bool TO_LOCAL, class A>
int frame_launch_dir(const A& a, hipStream_t s)
{
  bool vec = aligned16(a.nx) && aligned16(a.ny) && aligned16(a.nz) && aligned16(a.x) && aligned16(a.y) &&
                   aligned16(a.z) && aligned16(a.rx) && aligned16(a.ry) && aligned16(a.rz) &&
                   (reinterpret_cast<uintptr_t>(a.mask) & 3u) == 0;
  if constexpr (frame_tangent<A>) vec = vec && aligned16(a.tx) && aligned16(a.ty) && aligned16(a.tz);
  const unsigned blocks = var_blocks(vec ? (a.n >> 2) : a.n);
  if (blocks == 0) return var_launched(blocks);
  if (vec) hipLaunchKernelGGL((k_frame_v4<TO_LOCAL, A>), dim3(blocks), dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((k_frame_v1<TO_LOCAL, A>), dim3(blocks), dim3(kBlock), 0, s, a);
  return var_launched(blocks);
}

}  // namespace

int frame_launch(const FrameArgs& a, bool to_local, hipStream_t s)
{
  return to_local ? frame_launch_dir<true>(a, s) : frame_launch_dir<false>(a, s);
}

int frame_launch(const FrameTangentArgs& a, bool to_local, hipStream_t s)
{
  return to_local ? frame_launch_dir<true>(a, s) : frame_launch_dir<false>(a, s);
}

}  // namespace bbmhip
