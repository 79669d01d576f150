// render.h - the scene blob (minppo_amd/render.py scene_blob) as the renderer's host code (render.hip) and kernels (k_render.hip) see it.
//
// A little-endian blob of 4-byte words, in the style of the model blob: 16 header words
//   0 magic "MPSC", 1 version, 2 total words, 3 nq, 4 nbody, 5 njnt, 6 ngeom, 7 ncam, 8 has_plane, 9 plane_z (f32), 10 nface, 11 number of arrays, 12..15 zero
// then a directory of (offset in words, count) per array in the order of the enum below, then the arrays, each padded to 4 words.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mppo {

constexpr uint32_t kSceneMagic = 0x4353504Du;  // "MPSC"
constexpr uint32_t kSceneVersion = 1;
constexpr int kSceneHeaderWords = 16;
constexpr int kSceneMaxGeoms = 512;  // 24 words of LDS each: 48 KB
constexpr int kGeomWords = 24;       // a staged visual: pose 12 | type | size 3 | rgb 3 | bounding radius | hull face address, count | 2 spare
constexpr int kCamWords = 16;        // a frame's camera: position 3 | rotation 9 (row-major; its columns are the camera's x, y, z axes) | tan(fovy / 2) | 3 spare

enum SceneArray {
  SI_body_parent, SI_body_jntadr, SI_body_jntnum, SI_jnt_type, SI_jnt_qposadr, SI_geom_body, SI_geom_type, SI_geom_hull, SI_cam_body, SI_cam_mode,
  SF_body_pos, SF_body_quat, SF_jnt_pos, SF_jnt_axis, SF_qpos0, SF_geom_size, SF_geom_pos, SF_geom_mat, SF_geom_rgb, SF_geom_rbound, SF_hull_plane,
  SF_cam_pos, SF_cam_mat, SF_cam_tanhalf, SCENE_ARRAY_COUNT
};
constexpr int kSceneFirstFloat = SF_body_pos;

// geom types: MuJoCo's mjtGeom numbering (minppo_amd/model.py)
enum { RG_SPHERE = 2, RG_CAPSULE = 3, RG_ELLIPSOID = 4, RG_CYLINDER = 5, RG_BOX = 6, RG_MESH = 7 };
enum { CAM_FIXED = 0, CAM_TRACK = 1, CAM_UNSUPPORTED = 2 };

struct SceneView {
  int nq, nbody, njnt, ngeom, ncam, has_plane, nface;
  float plane_z;
  int o[SCENE_ARRAY_COUNT];  // word offset of every array
};

int32_t parse_scene_blob(const void* host_blob, size_t nbytes, SceneView* view);

int32_t render_poses_launch(const SceneView& v, const void* dev_blob, int F, const float* qpos, int q_ld, int camera, float* body_ws, float* pose, float* camw,
                            hipStream_t stream);
int32_t render_rays_launch(const SceneView& v, const void* dev_blob, int F, int W, int H, const float* pose, const float* camw, uint8_t* rgb, float* depth, int32_t* geom_id,
                           hipStream_t stream);

}  // namespace mppo
