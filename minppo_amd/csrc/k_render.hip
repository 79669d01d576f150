// k_render.hip - the two kernels of mppo_render (render.hip): what the reference leaves to MuJoCo's renderer (`env.render`, minppo/env.py:264-333).
//
//   render_poses  one thread per frame: forward kinematics of the scene's tree from that frame's qpos - bodies in index order, parents first; free, ball,
//                 hinge and slide joints; quaternions normalised as the environment kernel's kinematics normalises them - then the world pose of every
//                 visual (position + row-major rotation) and the frame's camera (position, basis, tan(fovy / 2)).
//   render_rays   256 threads per workgroup, one 16 x 16 pixel tile of one frame: wave w owns the 8 x 8 block (w & 1, w >> 1) of the tile, a lane one pixel.
//                 The workgroup stages its frame's visuals (24 words each) and camera into LDS once; every lane then casts one primary ray through its
//                 pixel centre and loops over ALL visuals, so the trip count, the LDS addresses and the shape-type switch are the same in every lane of a
//                 wave: the LDS reads are broadcasts, the switch is a scalar branch (the type goes through wave_uniform), and a hull's face planes are
//                 read from the blob at wave-uniform addresses.  Per shape the ray is taken into the geom's frame and intersected in closed form; a
//                 hit is the ray ENTERING a shape at t > 0.  Shading: Lambert from one directional light plus a constant ambient term, a hard shadow ray
//                 toward the light through the same routines, a two-tone 1 m checker on the ground, a constant sky.  One sample per pixel: the image is
//                 a pure function of the inputs.  Partial tiles: every lane computes (a clamped pixel), only lanes inside the image store.
//
// The quadratic is solved in its cancellation-free form: the discriminant comes from the squared distance of the centre to the ray (the point of
// closest approach), not from b * b - c.
#include <wave_ops.h>

#include <cmath>

#include "mppo_common.h"
#include "render.h"

namespace mppo {

namespace {

struct R3 { float x, y, z; };
struct RQ { float w, x, y, z; };
__device__ __forceinline__ R3 rld3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ RQ rld4(const float* p) { return {p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ R3 radd(R3 a, R3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ R3 rsub(R3 a, R3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ R3 rmul(R3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float rdot(R3 a, R3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ RQ rqmul(RQ a, RQ b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
__device__ __forceinline__ RQ rqnormalize(RQ q) {  // (k_physics.hip qnormalize)
  const float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  const float s = n > 0.f ? 1.f / n : 1.f;
  return {q.w * s, q.x * s, q.y * s, q.z * s};
}
__device__ __forceinline__ void rqmat(RQ q, float* m) {
  const float w = q.w, x = q.x, y = q.y, z = q.z;
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2.f * (x * y - w * z);         m[2] = 2.f * (x * z + w * y);
  m[3] = 2.f * (x * y + w * z);         m[4] = w * w - x * x + y * y - z * z; m[5] = 2.f * (y * z - w * x);
  m[6] = 2.f * (x * z - w * y);         m[7] = 2.f * (y * z + w * x);         m[8] = w * w - x * x - y * y + z * z;
}
// m v and m^T v for a row-major 3 x 3
__device__ __forceinline__ R3 rmatv(const float* m, R3 v) { return {m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z}; }
__device__ __forceinline__ R3 rmattv(const float* m, R3 v) { return {m[0] * v.x + m[3] * v.y + m[6] * v.z, m[1] * v.x + m[4] * v.y + m[7] * v.z, m[2] * v.x + m[5] * v.y + m[8] * v.z}; }
__device__ __forceinline__ R3 rqrot(RQ q, R3 v) {
  float m[9];
  rqmat(q, m);
  return rmatv(m, v);
}
__device__ __forceinline__ void rmatmul(const float* a, const float* b, float* c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

constexpr int kRenderThreads = 256;
constexpr int kPoseThreads = 64;

}  // namespace

__global__ void __launch_bounds__(kPoseThreads) render_poses_kernel(SceneView v, const void* __restrict__ blob, int F, const float* __restrict__ qpos_all, int q_ld, int camera,
                                                                    float* __restrict__ body_ws, float* __restrict__ pose_all, float* __restrict__ cam_all) {
  const int f = blockIdx.x * kPoseThreads + threadIdx.x;
  if (f >= F) return;
  const int32_t* bi = static_cast<const int32_t*>(blob);
  const float* bf = static_cast<const float*>(blob);
  const float* qpos = qpos_all + (size_t)f * q_ld;
  float* xb = body_ws + (size_t)f * v.nbody * 7;  // per body: position 3, quaternion 4
  xb[0] = 0.f; xb[1] = 0.f; xb[2] = 0.f; xb[3] = 1.f; xb[4] = 0.f; xb[5] = 0.f; xb[6] = 0.f;
  const int32_t *parent = bi + v.o[SI_body_parent], *jntadr = bi + v.o[SI_body_jntadr], *jntnum = bi + v.o[SI_body_jntnum], *jtype = bi + v.o[SI_jnt_type],
                *jqadr = bi + v.o[SI_jnt_qposadr];
  const float *body_pos = bf + v.o[SF_body_pos], *body_quat = bf + v.o[SF_body_quat], *jnt_pos = bf + v.o[SF_jnt_pos], *jnt_axis = bf + v.o[SF_jnt_axis], *qpos0 = bf + v.o[SF_qpos0];
  for (int b = 1; b < v.nbody; ++b) {
    const int p = parent[b];
    const RQ pq = rld4(xb + 7 * p + 3);
    R3 pos = radd(rld3(xb + 7 * p), rqrot(pq, rld3(body_pos + 3 * b)));
    RQ quat = rqmul(pq, rld4(body_quat + 4 * b));
    for (int j = jntadr[b], j1 = jntadr[b] + jntnum[b]; j < j1; ++j) {
      const int qa = jqadr[j], jt = jtype[j];
      if (jt == 0) {  // free
        pos = rld3(qpos + qa);
        quat = rqnormalize(rld4(qpos + qa + 3));
      } else {
        const R3 anchor = radd(pos, rqrot(quat, rld3(jnt_pos + 3 * j)));
        if (jt == 1) {  // ball: the hinge's form with the rotation taken from qpos
          quat = rqmul(quat, rqnormalize(rld4(qpos + qa)));
          pos = rsub(anchor, rqrot(quat, rld3(jnt_pos + 3 * j)));
        } else {
          const float disp = qpos[qa] - qpos0[qa];
          const R3 ax = rld3(jnt_axis + 3 * j);
          if (jt == 2) {  // hinge
            const float s = sinf(0.5f * disp), c = cosf(0.5f * disp);
            quat = rqmul(quat, RQ{c, s * ax.x, s * ax.y, s * ax.z});
            pos = rsub(anchor, rqrot(quat, rld3(jnt_pos + 3 * j)));
          } else {  // slide
            pos = radd(pos, rmul(rqrot(quat, ax), disp));
          }
        }
      }
    }
    quat = rqnormalize(quat);
    xb[7 * b] = pos.x; xb[7 * b + 1] = pos.y; xb[7 * b + 2] = pos.z;
    xb[7 * b + 3] = quat.w; xb[7 * b + 4] = quat.x; xb[7 * b + 5] = quat.y; xb[7 * b + 6] = quat.z;
  }
  // the visuals: world position + row-major rotation
  const int32_t* gbody = bi + v.o[SI_geom_body];
  const float *gpos = bf + v.o[SF_geom_pos], *gmat = bf + v.o[SF_geom_mat];
  float* pose = pose_all + (size_t)f * v.ngeom * 12;
  for (int g = 0; g < v.ngeom; ++g) {
    const int b = gbody[g];
    float rb[9], r[9];
    rqmat(rld4(xb + 7 * b + 3), rb);
    const R3 p = radd(rld3(xb + 7 * b), rmatv(rb, rld3(gpos + 3 * g)));
    rmatmul(rb, gmat + 9 * g, r);
    float* o = pose + 12 * g;
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    for (int k = 0; k < 9; ++k) o[3 + k] = r[k];
  }
  // the camera: fixed = rigid in its body's frame; track = offset from the body's position, orientation fixed in the world (both as the blob holds them)
  {
    const int b = (bi + v.o[SI_cam_body])[camera], mode = (bi + v.o[SI_cam_mode])[camera];
    const float *cpos = bf + v.o[SF_cam_pos] + 3 * camera, *cmat = bf + v.o[SF_cam_mat] + 9 * camera;
    float* o = cam_all + (size_t)f * kCamWords;
    R3 p;
    float r[9];
    if (mode == CAM_TRACK) {
      p = radd(rld3(xb + 7 * b), rld3(cpos));
      for (int k = 0; k < 9; ++k) r[k] = cmat[k];
    } else {
      float rb[9];
      rqmat(rld4(xb + 7 * b + 3), rb);
      p = radd(rld3(xb + 7 * b), rmatv(rb, rld3(cpos)));
      rmatmul(rb, cmat, r);
    }
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    for (int k = 0; k < 9; ++k) o[3 + k] = r[k];
    o[12] = (bf + v.o[SF_cam_tanhalf])[camera];
    o[13] = 0.f; o[14] = 0.f; o[15] = 0.f;
  }
}

namespace {

// the half space n . x <= off against the ray: denom = n . d, dist = off - n . o.  Keeps the latest entry (t0, its face) and the earliest exit (t1).
__device__ __forceinline__ bool clip_plane(float denom, float dist, float& t0, float& t1, int& face, int k) {
  if (denom < 0.f) {
    const float t = dist / denom;
    if (t > t0) { t0 = t; face = k; }
  } else if (denom > 0.f) {
    const float t = dist / denom;
    if (t < t1) t1 = t;
  } else if (dist < 0.f) {
    return false;
  }
  return true;
}

// entry of the ray o + t d into the sphere of radius^2 r2 about c; `a` = d . d.  Discriminant from the point of closest approach.
__device__ __forceinline__ bool sphere_entry(R3 o, R3 d, float a, R3 c, float r2, float& t) {
  const R3 oc = rsub(o, c);
  const float tc = -rdot(oc, d) / a;
  const R3 q = radd(oc, rmul(d, tc));
  const float q2 = rdot(q, q);
  if (q2 > r2) return false;
  t = tc - sqrtf((r2 - q2) / a);
  return true;
}

// The ray (o, d) in the geom's frame against one shape: the parameter at which it ENTERS (t > 0) and the outward normal there, in the geom's frame.
__device__ __forceinline__ bool intersect(int type, R3 sz, int hadr, int hcnt, const float* __restrict__ planes, R3 o, R3 d, float& t_hit, R3& n_hit) {
  const float inf = INFINITY;
  switch (type) {
    case RG_SPHERE:
    case RG_ELLIPSOID: {  // the unit sphere in the scaled frame
      const R3 os = {o.x / sz.x, o.y / sz.y, o.z / sz.z}, ds = {d.x / sz.x, d.y / sz.y, d.z / sz.z};
      float t;
      if (!sphere_entry(os, ds, rdot(ds, ds), R3{0.f, 0.f, 0.f}, 1.f, t) || !(t > 0.f)) return false;
      const R3 h = radd(os, rmul(ds, t));
      const R3 n = {h.x / sz.x, h.y / sz.y, h.z / sz.z};
      t_hit = t;
      n_hit = rmul(n, 1.f / sqrtf(rdot(n, n)));
      return true;
    }
    case RG_CAPSULE: {  // the cylinder's side between the caps' centres, and the two cap spheres: the earliest entry
      const float r = sz.x, hl = sz.y, r2 = r * r;
      float best = inf;
      R3 bn = {0.f, 0.f, 1.f};
      const float a = d.x * d.x + d.y * d.y;
      if (a > 0.f) {
        const float tc = -(o.x * d.x + o.y * d.y) / a;
        const float qx = o.x + tc * d.x, qy = o.y + tc * d.y;
        const float q2 = qx * qx + qy * qy;
        if (q2 > r2) return false;  // (the caps lie inside the infinite cylinder)
        const float t = tc - sqrtf((r2 - q2) / a);
        const float z = o.z + t * d.z;
        if (t > 0.f && fabsf(z) <= hl) { best = t; bn = R3{(o.x + t * d.x) / r, (o.y + t * d.y) / r, 0.f}; }
      }
      const float dd = rdot(d, d);
      for (int s = 0; s < 2; ++s) {
        const R3 c = {0.f, 0.f, s ? -hl : hl};
        float t;
        if (sphere_entry(o, d, dd, c, r2, t) && t > 0.f && t < best) {
          best = t;
          bn = rmul(rsub(radd(o, rmul(d, t)), c), 1.f / r);
        }
      }
      if (!(best < inf)) return false;
      t_hit = best;
      n_hit = bn;
      return true;
    }
    case RG_CYLINDER: {  // the infinite cylinder's interval clipped by the two cap planes
      const float r = sz.x, hl = sz.y, r2 = r * r;
      float t0 = -inf, t1 = inf;
      int face = 0;
      const float a = d.x * d.x + d.y * d.y;
      if (a > 0.f) {
        const float tc = -(o.x * d.x + o.y * d.y) / a;
        const float qx = o.x + tc * d.x, qy = o.y + tc * d.y;
        const float q2 = qx * qx + qy * qy;
        if (q2 > r2) return false;
        const float hh = sqrtf((r2 - q2) / a);
        t0 = tc - hh; t1 = tc + hh;
      } else if (o.x * o.x + o.y * o.y > r2) {
        return false;
      }
      if (!clip_plane(d.z, hl - o.z, t0, t1, face, 1) || !clip_plane(-d.z, hl + o.z, t0, t1, face, 2)) return false;
      if (!(t0 > 0.f) || !(t0 <= t1)) return false;
      t_hit = t0;
      n_hit = face == 0 ? R3{(o.x + t0 * d.x) / r, (o.y + t0 * d.y) / r, 0.f} : R3{0.f, 0.f, face == 1 ? 1.f : -1.f};
      return true;
    }
    case RG_BOX: {  // three slabs
      float t0 = -inf, t1 = inf;
      int face = 0;
      if (!clip_plane(d.x, sz.x - o.x, t0, t1, face, 0) || !clip_plane(-d.x, sz.x + o.x, t0, t1, face, 1) || !clip_plane(d.y, sz.y - o.y, t0, t1, face, 2) ||
          !clip_plane(-d.y, sz.y + o.y, t0, t1, face, 3) || !clip_plane(d.z, sz.z - o.z, t0, t1, face, 4) || !clip_plane(-d.z, sz.z + o.z, t0, t1, face, 5))
        return false;
      if (!(t0 > 0.f) || !(t0 <= t1)) return false;
      const float s = (face & 1) ? -1.f : 1.f;
      t_hit = t0;
      n_hit = R3{(face >> 1) == 0 ? s : 0.f, (face >> 1) == 1 ? s : 0.f, (face >> 1) == 2 ? s : 0.f};
      return true;
    }
    case RG_MESH: {  // the convex hull: the ray clipped against its face planes (global memory, the same address in every lane)
      float t0 = -inf, t1 = inf;
      int face = 0;
      const float* pl = planes + 4 * (size_t)hadr;
      for (int k = 0; k < hcnt; ++k) {
        const R3 n = rld3(pl + 4 * k);
        if (!clip_plane(rdot(n, d), pl[4 * k + 3] - rdot(n, o), t0, t1, face, k)) return false;
      }
      if (!(t0 > 0.f) || !(t0 <= t1)) return false;
      t_hit = t0;
      n_hit = rld3(pl + 4 * face);
      return true;
    }
    default:
      return false;
  }
}

__device__ __forceinline__ float to_level(float x) {  // [0, 1] -> 0 .. 255, round to nearest
  x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
  return floorf(x * 255.f + 0.5f);
}

}  // namespace

// light, shading and colours: fixed (the image is a function of the scene blob, qpos, the camera and the size alone)
#define RENDER_LIGHT R3{2.f / 7.f, -3.f / 7.f, 6.f / 7.f}  /* a unit vector toward the light */
constexpr float kAmbient = 0.35f, kDiffuse = 0.65f, kShadowBias = 1e-3f;

__global__ void __launch_bounds__(kRenderThreads) render_rays_kernel(SceneView v, const void* __restrict__ blob, int W, int H, int tiles_x, int tiles_per_frame,
                                                                     const float* __restrict__ pose_all, const float* __restrict__ cam_all, unsigned char* __restrict__ rgb,
                                                                     float* __restrict__ depth, int32_t* __restrict__ geom_id) {
  MPPO_DYN_SMEM(smem);
  float* sg = reinterpret_cast<float*>(smem);  // [ngeom][kGeomWords], then the camera
  const int ng = v.ngeom;
  float* scam = sg + (size_t)ng * kGeomWords;
  const int32_t* bi = static_cast<const int32_t*>(blob);
  const float* bf = static_cast<const float*>(blob);
  const int f = blockIdx.x / tiles_per_frame, tile = blockIdx.x % tiles_per_frame;
  const int tid = threadIdx.x;
  {
    const float* pose = pose_all + (size_t)f * ng * 12;
    const int32_t *gtype = bi + v.o[SI_geom_type], *ghull = bi + v.o[SI_geom_hull];
    const float *gsize = bf + v.o[SF_geom_size], *grgb = bf + v.o[SF_geom_rgb], *grb = bf + v.o[SF_geom_rbound];
    for (int g = tid; g < ng; g += kRenderThreads) {
      float* d = sg + kGeomWords * g;
      for (int k = 0; k < 12; ++k) d[k] = pose[12 * g + k];
      d[12] = __uint_as_float((unsigned)(gtype[g]));
      for (int k = 0; k < 3; ++k) { d[13 + k] = gsize[3 * g + k]; d[16 + k] = grgb[3 * g + k]; }
      d[19] = grb[g];
      d[20] = __uint_as_float((unsigned)(ghull[2 * g]));
      d[21] = __uint_as_float((unsigned)(ghull[2 * g + 1]));
      d[22] = 0.f; d[23] = 0.f;
    }
    if (tid < kCamWords) scam[tid] = cam_all[(size_t)f * kCamWords + tid];
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int px = (tile % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7), py = (tile / tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool inside = px < W && py < H;
  const int cx = px < W ? px : W - 1, cy = py < H ? py : H - 1;  // (a masked lane casts its neighbour's ray: every lane runs the same loops)
  // MuJoCo's camera: looks along -z, +x right, +y up, vertical field of view
  const float th = scam[12];
  const R3 dc = {(2.f * ((float)cx + 0.5f) / (float)W - 1.f) * th * ((float)W / (float)H), (1.f - 2.f * ((float)cy + 0.5f) / (float)H) * th, -1.f};
  const R3 org = rld3(scam);
  R3 dir = rmatv(scam + 3, dc);
  dir = rmul(dir, 1.f / sqrtf(rdot(dir, dir)));
  const float* planes = bf + v.o[SF_hull_plane];

  float best = INFINITY;
  int id = -1;
  R3 bn = {0.f, 0.f, 1.f};
  for (int g = 0; g < ng; ++g) {
    const float* s = sg + kGeomWords * g;
    const int type = wave_uniform((int)__float_as_uint(s[12])), hadr = wave_uniform((int)__float_as_uint(s[20])), hcnt = wave_uniform((int)__float_as_uint(s[21]));
    const R3 ol = rmattv(s + 3, rsub(org, rld3(s))), dl = rmattv(s + 3, dir);
    float t;
    R3 n;
    if (intersect(type, rld3(s + 13), hadr, hcnt, planes, ol, dl, t, n) && t < best) {
      best = t;
      id = g;
      bn = rmatv(s + 3, n);
    }
  }
  if (v.has_plane && dir.z != 0.f) {
    const float t = (v.plane_z - org.z) / dir.z;
    if (t > 0.f && t < best) { best = t; id = ng; bn = R3{0.f, 0.f, 1.f}; }
  }
  R3 col = {0.55f, 0.70f, 0.90f};  // the sky
  if (id >= 0) {
    const R3 light = RENDER_LIGHT;
    const R3 hit = radd(org, rmul(dir, best));
    R3 base;
    if (id == ng) {  // the ground: a two-tone checker of 1 m cells
      const int cell = (int)floorf(hit.x) + (int)floorf(hit.y);
      base = (cell & 1) ? R3{0.45f, 0.50f, 0.55f} : R3{0.75f, 0.75f, 0.75f};
    } else {
      base = rld3(sg + kGeomWords * id + 16);
    }
    float lit = rdot(bn, light);
    lit = lit > 0.f ? lit : 0.f;
    if (lit > 0.f) {  // a hard shadow: anything the ray toward the light enters
      const R3 so = radd(hit, rmul(bn, kShadowBias));
      bool shadow = false;
      for (int g = 0; g < ng; ++g) {
        const float* s = sg + kGeomWords * g;
        const int type = wave_uniform((int)__float_as_uint(s[12])), hadr = wave_uniform((int)__float_as_uint(s[20])), hcnt = wave_uniform((int)__float_as_uint(s[21]));
        const R3 ol = rmattv(s + 3, rsub(so, rld3(s))), dl = rmattv(s + 3, light);
        float t;
        R3 n;
        shadow = shadow || intersect(type, rld3(s + 13), hadr, hcnt, planes, ol, dl, t, n);
      }
      if (shadow) lit = 0.f;
    }
    const float k = kAmbient + kDiffuse * lit;
    col = rmul(base, k);
  }
  if (inside) {
    const size_t pix = ((size_t)f * H + py) * W + px;
    if (rgb) {
      rgb[3 * pix] = (unsigned char)to_level(col.x);
      rgb[3 * pix + 1] = (unsigned char)to_level(col.y);
      rgb[3 * pix + 2] = (unsigned char)to_level(col.z);
    }
    if (depth) depth[pix] = best;
    if (geom_id) geom_id[pix] = id;
  }
}

int32_t render_poses_launch(const SceneView& v, const void* dev_blob, int F, const float* qpos, int q_ld, int camera, float* body_ws, float* pose, float* camw,
                            hipStream_t stream) {
  hipLaunchKernelGGL(render_poses_kernel, dim3(cdiv(F, kPoseThreads)), dim3(kPoseThreads), 0, stream, v, dev_blob, F, qpos, q_ld, camera, body_ws, pose, camw);
  MPPO_CHECK_LAUNCH("render_poses_kernel");
  return MPPO_OK;
}

int32_t render_rays_launch(const SceneView& v, const void* dev_blob, int F, int W, int H, const float* pose, const float* camw, uint8_t* rgb, float* depth, int32_t* geom_id,
                           hipStream_t stream) {
  const int tiles_x = cdiv(W, 16), tiles_y = cdiv(H, 16);
  const long blocks = (long)tiles_x * tiles_y * F;
  MPPO_REQUIRE(blocks <= 0x7fffffffL, "mppo_render: %ld tiles exceed one launch", blocks);
  const size_t lds = ((size_t)v.ngeom * kGeomWords + kCamWords) * sizeof(float);
  hipLaunchKernelGGL(render_rays_kernel, dim3((unsigned)blocks), dim3(kRenderThreads), lds, stream, v, dev_blob, W, H, tiles_x, tiles_x * tiles_y, pose, camw, rgb, depth, geom_id);
  MPPO_CHECK_LAUNCH("render_rays_kernel");
  return MPPO_OK;
}

}  // namespace mppo
