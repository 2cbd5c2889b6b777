/*
 * pthost.h -- headless host side of the path tracer: the counterpart of the
 * reference's scene loader (src/scene.cpp, src/utilities.cpp:65-72), of the camera set-up that
 * runCuda performs before the first pathtrace() (src/main.cpp:53-67,102-120) and of saveImage /
 * image::savePNG (src/main.cpp:78-99, src/image.cpp:22-39).  Plain C ABI so that tests can drive
 * it through ctypes; structs are the C-ABI mirrors of include/ptmi355.h.
 */
#ifndef PTHOST_H
#define PTHOST_H

#include "../../include/ptmi355.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pth_scene {
    pt_geom *geoms;          int32_t num_geoms;
    pt_material *materials;  int32_t num_materials;
    pt_triangle *triangles;  int32_t num_triangles;   /* "mesh" objects (format extension) */
    pt_mesh *meshes;         int32_t num_meshes;
    pt_camera camera_loaded;   /* exactly as Scene::loadCamera leaves it (right = NaN, scene.cpp:138) */
    pt_camera camera;          /* after the runCuda orbit recompute: what the kernels must see */
    int32_t iterations;        /* ITERATIONS */
    int32_t trace_depth;       /* DEPTH */
    char image_name[256];      /* FILE */
} pth_scene;

/* Scene::Scene(filename) (scene.cpp:7-33).  Returns NULL and sets pth_last_error() on failure. */
pth_scene *pth_load_scene(const char *path);
void pth_free_scene(pth_scene *s);
const char *pth_last_error(void);
/* The scene's cube textures (format extension; include/ptmi355.h "texture mapping"): a top-level block
 *   TEXTURE <material id>
 *   CHECKER <n> <cells> r0 g0 b0 r1 g1 b1   |   PFM <file>
 * CHECKER: texel (face, j, i) takes colour 0 or 1 by the parity of i * cells / n + j * cells / n + face (integer arithmetic);
 * PFM: a colour PFM n wide and 6 n tall, faces 0..5 top to bottom, relative to the scene's directory.  *n = the size of that
 * material's texture (0: none), *texels = its 6 * n * n RGB triples (owned by the scene; NULL when none).  0, or -1 for a bad
 * argument. */
int pth_scene_texture(const pth_scene *s, int material, const float **texels, int *n);
/* ... and its cube bump maps (include/ptmi355.h "bump mapping"): a top-level block
 *   BUMPMAP <material id>
 *   STUDS <n> <cells> <slope>   |   PFM <file>
 * STUDS, integer arithmetic only: for texel (face, j, i), pa = (i * cells * 4 / n) % 4 and sa = -1, 0, 0, 1 for pa = 0..3, sb
 * likewise from j; the texel is (slope * sa, slope * sb, 0) -- bevelled studs, every value 0 or +-slope exactly.  PFM as for
 * TEXTURE, a texel (da, db, unused).  The accessor has pth_scene_texture's contract. */
int pth_scene_bump_map(const pth_scene *s, int material, const float **texels, int *n);
/* ... and the per-vertex normals of its meshes (include/ptmi355.h "smooth shading"): the loader keeps the `vn` lines of a mesh
 * file and the third index of `i//k` and `i/j/k` face entries.  Each vn becomes multiplyMV(invTranspose, (vn, 0)) of the mesh's
 * geom, normalised in binary32; a triangle with a corner that names no normal gets three zero normals ("stays faceted").
 * *num_triangles = the scene's num_triangles and *normals = nine floats per triangle in the order of pth_scene::triangles
 * (owned by the scene) -- or 0 and NULL when no mesh file carried a `vn` line.  0, or -1 for a bad argument. */
int pth_scene_vertex_normals(const pth_scene *s, const float **normals, int *num_triangles);

/* utilityCore::buildTransformationMatrix (utilities.cpp:65-72) + glm::inverse + glm::inverseTranspose
 * (scene.cpp:82-85), GLM 0.9.6.3 operation order */
void pth_build_geom_matrices(pt_geom *g);

/* saveImage + image::savePNG: pixel = sum / samples, x-flip, clamp [0,1], * 255.f, truncate.
 * rgb_out: W*H*3 bytes in file order. */
void pth_image_to_rgb8(const float *image_sum, int w, int h, float samples, uint8_t *rgb_out);
int pth_write_png(const char *path, const uint8_t *rgb, int w, int h);          /* stored-deflate PNG */
int pth_write_pfm(const char *path, const float *image_sum, int w, int h, float samples);
/* the floats of a little-endian colour PFM of exactly w x h pixels (times |scale|), rows top to bottom as in memory:
 * with samples = 1 on the writing side this is the running sum itself (the reference keeps nothing else between
 * iterations, pathtrace.cu:71,84,389), exact */
int pth_read_pfm(const char *path, float *image_sum, int w, int h);

#ifdef __cplusplus
}
#endif
#endif
