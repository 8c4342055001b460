// bbm_amd/csrc/frame.hpp -- the reference's shading frame (core/shading_frame.h:26-58, Duff et al. 2017's basis)
// as one device struct: the arithmetic sphere_pixel (image.hpp), the lobes' to_global (lobes.hpp) and the frame
// kernels (frame.hip, and the world-space sample_eval kernels of sample_eval.hpp) share.
//
// toGlobalShadingFrame(n) is the matrix with columns X, Y, Z, Z = normalize(n); to_global is M v and to_local is
// transpose(M) v (toLocalShadingFrame).  X and Y are filled in one of two ways:
//   shading_frame(n)      from the normal alone (Duff et al.), the reference's frame;
//   tangent_frame(n, t)   from the normal and a world-space tangent t of any length, for the models
//                         whose parameters run along X and Y.  Z, rn and live are shading_frame(n)'s.  With
//                         d = dot3(Z, t), p = t - Z * d and pp = dot3(p, p): where pp > epsilon (tangent_live; a NaN
//                         is not), X = p * (1 / sqrt(pp)) and Y = cross(Z, X), right-handed (X x Y = Z) as the Duff
//                         frame is; elsewhere -- a zero tangent, one parallel to the normal, one shorter than about
//                         3.5e-4, a NaN -- the frame is shading_frame(n)'s, bit for bit.
#pragma once
#include "math.hpp"

namespace bbmhip {

struct Frame
{
  v3 X, Y, Z;
  bool live;      // |n|^2 > epsilon; X, Y, Z of a frame that is not live hold nothing to use

  // transpose(mat3d(X, Y, Z)) * v: row r of the transpose is column r, one dot per row (core/mat.h:107-116)
  __device__ __forceinline__ v3 to_local(v3 v) const { return mk3(dot3(X, v), dot3(Y, v), dot3(Z, v)); }
  // mat3d * v: row r = (X[r], Y[r], Z[r]) dotted with v
  __device__ __forceinline__ v3 to_global(v3 v) const
  {
    return mk3(row_dot(X.x * v.x, Y.x * v.y, Z.x * v.z), row_dot(X.y * v.x, Y.y * v.y, Z.y * v.z),
               row_dot(X.z * v.x, Y.z * v.y, Z.z * v.z));
  }

  // ((0 + a) + b) + c, the reference's sum (core/mat.h:107-116), written without its leading zero: the two differ only
  // where a, b and c are all -0, where the reference's is +0, and a sum that is 0 can be -0 in no other way.  The
  // literal form is not safe here: X.z is a negation, `0 + (-p)` becomes `0 - p`, and instruction selection may fold
  // that into a negated operand of the next sum -- -0 for p = +0 -- in one kernel and not in another (seen: a failed
  // sample's zero direction came back as z = -0 from the frame kernel and +0 from the fused one).
  __device__ __forceinline__ static float row_dot(float a, float b, float c)
  {
    const float r = (a + b) + c;
    return r == 0.0f ? 0.0f : r;
  }
};

// The frame of the normal n, rn = 1 / |n| formed by the caller: Z = normalize(n) = n * (1 / sqrt(|n|^2)).  The double
// literals (-1.0 / (sign + z), 1.0 + ...) widen one float operand, and one double operation rounded to float is the
// float operation (53 >= 2 x 24 + 2), so everything is float arithmetic.
__device__ __forceinline__ Frame frame_scaled(v3 n, float rn, bool live)
{
  const v3 Z = mk3(n.x * rn, n.y * rn, n.z * rn);
  const float sign = copysignf(1.0f, Z.z);
  const float a = div_nr(-1.0f, sign + Z.z);
  const float b = (Z.x * Z.y) * a;
  return Frame{mk3(1.0f + ((sign * Z.x) * Z.x) * a, sign * b, (-sign) * Z.x), mk3(b, sign + (Z.y * Z.y) * a, -Z.y), Z,
               live};
}

// The frame of a shading normal of any length, as renderSphere builds it (renderSphere.cpp:46-52): live where
// |n|^2 > epsilon (a NaN normal is not).
__device__ __forceinline__ Frame shading_frame(v3 n)
{
  const float nn = dot3(n, n);
  return frame_scaled(n, div_nr(1.0f, sqrt_nr(nn)), nn > kEpsF);
}

// The frame of a shading normal and a tangent, both of any length (the rule is at the head of this file): t's part
// perpendicular to the normal, normalized, is X; where it has none to speak of the frame is shading_frame(n)'s.
__device__ __forceinline__ Frame tangent_frame(v3 n, v3 t)
{
  const Frame f = shading_frame(n);
  const v3 Z = f.Z;
  const float d = dot3(Z, t);
  const v3 p = mk3(t.x - Z.x * d, t.y - Z.y * d, t.z - Z.z * d);
  const float pp = dot3(p, p);
  const bool tangent_live = pp > kEpsF;
  const float rp = div_nr(1.0f, sqrt_nr(pp));
  const v3 X = mk3(p.x * rp, p.y * rp, p.z * rp);
  const v3 Y = cross3(Z, X);
  return Frame{tangent_live ? X : f.X, tangent_live ? Y : f.Y, Z, f.live};
}

// the frame of a lane: the tangent is looked at only where the kernel was built with one
template<bool TANGENT>
__device__ __forceinline__ Frame lane_shading_frame(v3 n, v3 t)
{
  if constexpr (TANGENT) return tangent_frame(n, t);
  else return shading_frame(n);
}

// One lane of the frame calls: the vector in the other frame, 0 where the lane is masked or its frame is not live.
template<bool TO_LOCAL, bool TANGENT = false>
__device__ __forceinline__ v3 frame_apply(v3 n, v3 v, bool active, v3 t = mk3(0.0f, 0.0f, 0.0f))
{
  const Frame f = lane_shading_frame<TANGENT>(n, t);
  const v3 r = TO_LOCAL ? f.to_local(v) : f.to_global(v);
  return (active && f.live) ? r : mk3(0.0f, 0.0f, 0.0f);
}

struct FrameArgs
{
  const float* nx; const float* ny; const float* nz;   // the shading normal per lane, any length
  const float* x; const float* y; const float* z;
  const uint8_t* mask;                                 // or nullptr
  uint64_t n;
  float* rx; float* ry; float* rz;
};
// the tangent frame calls (bbm_hip_frame_to_local_tangent / _to_global_tangent)
struct FrameTangentArgs : FrameArgs
{
  const float* tx; const float* ty; const float* tz;   // the tangent per lane, any length
};

int frame_launch(const FrameArgs& a, bool to_local, hipStream_t s);     // frame.hip
int frame_launch(const FrameTangentArgs& a, bool to_local, hipStream_t s);

}  // namespace bbmhip
