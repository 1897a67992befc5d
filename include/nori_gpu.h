/*
 * nori_gpu.h -- C ABI of the MI355X wavefront path tracer (libnori_gpu.so).
 *
 * This is the drop-in boundary for Nori's render path.  The reference binds
 * the path through C++ virtuals, not an FFI; each entry point below names the
 * reference interface it replaces (paths relative to the reference checkout):
 *
 *   nori_scene_load_xml   <- loadFromXML()                src/parser.cpp:28-338
 *                            + NoriObjectFactory::createInstance  include/nori/object.h:160-165
 *                            + Scene::activate()          src/scene.cpp:43-61
 *   nori_gpu_create       <- Scene::activate's BVH::build src/bvh.cpp:329-382 (flatten + upload)
 *                            and Integrator::preprocess    src/photonmapper.cpp:41-117 (photon map)
 *   nori_gpu_render       <- RenderThread::renderScene's pass loop
 *                            src/render.cpp:173-250 (tbb::parallel_for over blocks,
 *                            renderBlock render.cpp:80-133, Integrator::Li
 *                            include/nori/integrator.h:55, ImageBlock::put
 *                            src/block.cpp:93-133)
 *   nori_gpu_trace        <- Scene::rayIntersect(ray, its) / rayIntersect(ray)
 *                            include/nori/scene.h:93-115 -> BVH::rayIntersect src/bvh.cpp:404-462
 *   nori_gpu_query        <- Scene::rayIntersect(ray, its) with the whole Intersection
 *                            include/nori/scene.h:93-115 + setHitInformation
 *                            src/mesh.cpp:122-170, src/sphere.cpp:78-93
 *                            (nori_scene_surface: the same record on the host)
 *   nori_gpu_camera_rays  <- Camera::sampleRay src/perspective.cpp:90-112,
 *                            src/thinlens.cpp:120-147, src/advancedCamera.cpp:85-157
 *   nori_gpu_li           <- Integrator::Li include/nori/integrator.h:55 (a batch of
 *                            the caller's rays; src/path_mis.cpp, path_mats.cpp,
 *                            volumetric.cpp, direct*.cpp, normals.cpp,
 *                            averagevisibility.cpp, photonmapper.cpp)
 *   nori_gpu_cancel       <- RenderThread::stopRendering  src/render.cpp:63-71
 *   nori_gpu_progress     <- RenderThread::getProgress    src/render.cpp:73-78
 *   nori_film_develop     <- ImageBlock::toBitmap         src/block.cpp:76-82
 *   nori_write_exr        <- Bitmap::save                 src/bitmap.cpp:82-107
 *   nori_read_exr         <- Bitmap::Bitmap(filename)     src/bitmap.cpp:23-80
 *   nori_read_image       <- stbi_load in ImageTexture / NormalMap  src/imagetexture.cpp:69-85
 *   nori_write_png        <- Bitmap::saveToLDR            src/bitmap.cpp:122-139
 *   nori_film_variance    <- renderScene's variance image src/render.cpp:164-169,190-245
 *   nori_denoise          <- denoiser/denoiser.py:53-66 (NL-means)
 *   nori_film_block_error, nori_gpu_block_error, nori_gpu_render_adaptive
 *                         (adaptive sampling: no reference counterpart, the
 *                          reference gives every pixel sampleCount passes)
 *   nori_gpu_render_features, nori_film_features, nori_film_denoise_guided,
 *   nori_denoise_guided   (first-hit feature buffers and the feature-guided
 *                          denoiser: no reference counterpart, the reference
 *                          writes radiance and its variance image only)
 *   nori_scene_bvh_info   <- BVH::build/statistics        src/bvh.cpp:329-402
 *   nori_scene_scan_list  (introspection: the small-scene scan list and its
 *                          exact in-plane filters, for the CPU tests)
 *   nori_gpu_update_vertices, nori_scene_bvh_refit, nori_gpu_bvh_read
 *                         (dynamic geometry: new vertex positions and a BVH
 *                          refit on the device; no reference counterpart, the
 *                          reference builds its BVH once in Scene::activate)
 *   nori_gpu_rebuild_bvh, nori_scene_bvh_rebuild
 *                         (dynamic geometry: a linear BVH built on the device
 *                          for the positions as they are now; no reference
 *                          counterpart)
 *   nori_scene_surface_grad, nori_gpu_surface_grad
 *                         (the hit record's adjoint in the vertex positions and
 *                          normals; no reference counterpart)
 *   nori_scene_materials, nori_scene_bsdf_grad, nori_gpu_update_materials,
 *   nori_gpu_materials, nori_gpu_bsdf_grad
 *                         (differentiable materials: BSDF parameters set on a
 *                          live context, and bsdf_eval's adjoint in them; no
 *                          reference counterpart)
 *   nori_scene_scan_rtc, nori_scene_shade_rtc, nori_gpu_shade_rtc_info
 *                         (the scene-specialised kernels compiled at context
 *                          creation through hipRTC; no reference counterpart)
 *   nori_gpu_comm_*, nori_gpu_render_sharded
 *                         <- the same pass loop spread over the GPUs of a node,
 *                            one process per GPU; the cross-GPU film merge is
 *                            ImageBlock::put(block) src/block.cpp:124-133 as an
 *                            RCCL sum over xGMI (the reference has no multi-device path)
 *
 * Rules of the ABI: plain C types only, no exceptions cross it, every call
 * returns an int status (NORI_OK = 0, negative = error) and the message of
 * the last failure on the calling thread is nori_gpu_last_error().  All
 * scene arrays are copied at nori_gpu_create(); the caller owns output
 * buffers.  Arithmetic on the path is fp32 (Eigen float in the reference).
 */
#ifndef NORI_GPU_H
#define NORI_GPU_H

#ifndef __HIPCC_RTC__  /* (the library compiles its scan kernels at run time with hipRTC, which has size_t built in) */
#include <stddef.h>
#endif
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an exported signature or a shared struct changes (6: the
 * leading status argument of nori_gpu_comm_timeout; 7: nori_gpu_stats.nee_inline);
 * the Python binding and the C++ adapter refuse a library of another version. */
#define NORI_GPU_ABI_VERSION 7

/* ---- status codes ------------------------------------------------------ */
#define NORI_OK               0
#define NORI_ERR_INVALID     -1   /* bad argument                        */
#define NORI_ERR_IO          -2   /* file could not be read / written    */
#define NORI_ERR_PARSE       -3   /* XML / OBJ syntax or property error  */
#define NORI_ERR_UNSUPPORTED -4   /* plugin outside this path's scope    */
#define NORI_ERR_HIP         -5   /* HIP runtime failure / no device     */
#define NORI_ERR_CANCELLED   -6   /* nori_gpu_cancel() was honoured      */
#define NORI_ERR_OOM         -7   /* device allocation failed            */

/* ---- plugin kinds (XML `type` names in comments) ------------------------ */
enum { NORI_SHAPE_MESH = 0 /* "obj" */, NORI_SHAPE_SPHERE = 1 /* "sphere" */ };
enum {
    NORI_BSDF_DIFFUSE = 0,    /* "diffuse"    src/diffuse.cpp    */
    NORI_BSDF_MIRROR = 1,     /* "mirror"     src/mirror.cpp     */
    NORI_BSDF_DIELECTRIC = 2, /* "dielectric" src/dielectric.cpp */
    NORI_BSDF_MICROFACET = 3, /* "microfacet" src/microfacet.cpp */
    NORI_BSDF_DISNEY = 4      /* "disney"     src/disney.cpp     */
};
enum {
    NORI_EMITTER_AREA = 0,    /* "area"      src/arealight.cpp  */
    NORI_EMITTER_ENVMAP = 1,  /* "envmap"    src/envmap.cpp     */
    NORI_EMITTER_POINT = 2,   /* "point"     src/pointlight.cpp */
    NORI_EMITTER_SPOT = 3     /* "spotlight" src/spotlight.cpp  */
};
enum {
    NORI_TEXTURE_CONSTANT = 0,     /* "constant_color"     src/consttexture.cpp */
    NORI_TEXTURE_CHECKERBOARD = 1, /* "checkerboard_color" src/checkerboard.cpp */
    NORI_TEXTURE_IMAGE = 2         /* "ImageTexture"       src/imagetexture.cpp */
};
/* ImageWrap (include/nori/common.h:273-283): "repeat" | "clamp" */
enum { NORI_WRAP_REPEAT = 0, NORI_WRAP_CLAMP = 1 };
enum {
    NORI_CAMERA_PERSPECTIVE = 0,   /* "perspective"    src/perspective.cpp    */
    NORI_CAMERA_THINLENS = 1,      /* "thinlens"       src/thinlens.cpp       */
    NORI_CAMERA_ADVANCED = 2       /* "advancedCamera" src/advancedCamera.cpp */
};
enum {
    NORI_INTEGRATOR_PATH_MATS = 0,  /* "path_mats"  src/path_mats.cpp  */
    NORI_INTEGRATOR_PATH_MIS = 1,   /* "path_mis"   src/path_mis.cpp   */
    NORI_INTEGRATOR_VOLUMETRIC = 2, /* "volumetric" src/volumetric.cpp */
    /* one-bounce integrators (a fixed number of rays per camera sample) */
    NORI_INTEGRATOR_NORMALS = 3,    /* "normals"     src/normals.cpp           */
    NORI_INTEGRATOR_AV = 4,         /* "av"          src/averagevisibility.cpp */
    NORI_INTEGRATOR_DIRECT = 5,     /* "direct"      src/direct.cpp            */
    NORI_INTEGRATOR_DIRECT_EMS = 6, /* "direct_ems"  src/direct_ems.cpp        */
    NORI_INTEGRATOR_DIRECT_MATS = 7,/* "direct_mats" src/direct_mats.cpp       */
    NORI_INTEGRATOR_DIRECT_MIS = 8, /* "direct_mis"  src/direct_mis.cpp        */
    NORI_INTEGRATOR_PHOTONMAPPER = 9 /* "photonmapper" src/photonmapper.cpp    */
};
enum {
    NORI_FILTER_GAUSSIAN = 0, NORI_FILTER_MITCHELL = 1, NORI_FILTER_TENT = 2,
    NORI_FILTER_BOX = 3, NORI_FILTER_WINDOWED = 4     /* src/rfilter.cpp */
};
/* Random-number stream layout.
 *  WAVE : one pcg32 stream per (pass k, pixel) sample -- counter based, the
 *         layout the GPU uses; identical in the CPU oracle.
 *  BLOCK: the reference's layout: one stream per 32x32 block seeded with
 *         seed(offset.x, offset.y) and consumed serially over pixels and
 *         passes (src/independent.cpp:48-67, src/render.cpp:212-216).  CPU
 *         oracle only. */
enum { NORI_RNG_WAVE = 0, NORI_RNG_BLOCK = 1 };

#define NORI_BLOCK_SIZE 32           /* include/nori/block.h:30   */
#define NORI_FILTER_RESOLUTION 32    /* include/nori/rfilter.h:25 */
#define NORI_EPSILON 1e-4f           /* include/nori/common.h:52  */

/* ---- flattened scene (POD) ---------------------------------------------- */
typedef struct nori_shape_desc {
    int32_t type;                 /* NORI_SHAPE_*                              */
    uint32_t tri_offset;          /* mesh: first triangle in indices[]         */
    uint32_t tri_count;           /* mesh: triangle count (sphere: 1 primitive) */
    uint32_t vtx_offset;          /* mesh: first vertex in positions[]         */
    uint32_t vtx_count;
    int32_t has_normals;          /* mesh: per-vertex normals present          */
    int32_t has_uvs;              /* mesh: per-vertex uvs present              */
    float center[3];              /* sphere                                    */
    float radius;                 /* sphere                                    */
    int32_t bsdf;                 /* index into bsdfs[]                         */
    int32_t emitter;              /* index into emitters[] or -1               */
    int32_t normal_map;           /* "NormalMap" texture named "normal": index
                                     into images[] or -1 (shape.cpp:59-67;
                                     applied to meshes with normals, mesh.cpp:147-155) */
} nori_shape_desc;

typedef struct nori_bsdf_desc {
    int32_t type;                 /* NORI_BSDF_*                               */
    float albedo[3];              /* diffuse: constant_color albedo (def 0.5)  */
    float int_ior, ext_ior;       /* dielectric / microfacet                   */
    float alpha;                  /* microfacet                                */
    float kd[3];                  /* microfacet                                */
    float base_color[3];          /* disney                                    */
    float metallic, specular, roughness, sheen, sheen_tint, specular_tint;
    int32_t albedo_texture;       /* diffuse: NORI_TEXTURE_* of the albedo; a
                                     checkerboard uses albedo as value1        */
    float tex_value2[3];          /* checkerboard value2                        */
    float tex_delta[2], tex_scale[2]; /* checkerboard delta (def 0), scale (def 1) */
    int32_t albedo_image;         /* NORI_TEXTURE_IMAGE: index into images[], else -1 */
} nori_bsdf_desc;

/* An 8-bit RGB image of an ImageTexture or NormalMap, as stbi_load(path, ..,
 * STBI_rgb) returns it: width x height x 3 bytes, top row first. */
typedef struct nori_image_desc {
    int32_t width, height;
    int32_t wrap;                 /* NORI_WRAP_*                                */
    const uint8_t *rgb;
} nori_image_desc;

typedef struct nori_emitter_desc {
    int32_t type;                 /* NORI_EMITTER_*                            */
    int32_t shape;                /* attached shape index (area, envmap)       */
    float radiance[3];            /* area                                      */
    float weight;                 /* envmap                                    */
    float lum_scale[3];           /* envmap luminanceScale                     */
    int32_t env_rows, env_cols;   /* envmap: Bitmap rows x cols                */
    const float *env_rgb;         /* envmap: rows*cols*3 floats (row-major)    */
    float position[3];            /* point / spot                              */
    float power[3];               /* point: power | spot: color                */
    float direction[3];           /* spot: normalized direction                */
    float cos_falloff_start;      /* spot: cos(falloffStart deg)               */
    float cos_total_width;        /* spot: cos(totalWidth deg)                 */
} nori_emitter_desc;

typedef struct nori_camera_desc {
    int32_t width, height;
    float fov, near_clip, far_clip;
    float camera_to_world[16];    /* row-major 4x4                             */
    float sample_to_camera[16];   /* row-major 4x4 (perspective.cpp:53-82)     */
    int32_t filter_type;          /* NORI_FILTER_*                             */
    float filter_radius;
    float filter_p0, filter_p1;   /* gaussian: stddev | mitchell: B, C | windowed: tau */
    int32_t camera_type;          /* NORI_CAMERA_*                             */
    float lens_radius;            /* thinlens / advancedCamera "lensRadius"    */
    float focal_distance;         /* "focalDist"                               */
    float distortion[2];          /* advancedCamera barrel distortion k1, k2   */
    float chromatic[3];           /* advancedCamera "chromaticAberation"       */
} nori_camera_desc;

typedef struct nori_medium_desc {
    int32_t present;
    float sigma_a[3], sigma_s[3];
    float box_min[3], box_max[3]; /* origin -/+ |box_size| (medium.cpp:16-18)  */
} nori_medium_desc;

typedef struct nori_scene_desc {
    uint32_t abi_version;
    uint32_t num_vertices;
    const float *positions;       /* 3*num_vertices                            */
    const float *normals;         /* 3*num_vertices (zeros where absent)       */
    const float *uvs;             /* 2*num_vertices (zeros where absent)       */
    uint32_t num_triangles;
    const uint32_t *indices;      /* 3*num_triangles, global vertex ids        */
    uint32_t num_shapes;
    const nori_shape_desc *shapes;      /* BVH primitive order = shape order  */
    uint32_t num_bsdfs;
    const nori_bsdf_desc *bsdfs;
    uint32_t num_emitters;
    const nori_emitter_desc *emitters;  /* Scene::addChild order (scene.cpp:63-104) */
    nori_camera_desc camera;
    nori_medium_desc medium;
    int32_t integrator;           /* NORI_INTEGRATOR_*                          */
    uint32_t sample_count;        /* independent sampler sampleCount = spp      */
    float av_length;              /* "av" integrator ray length                 */
    uint32_t photon_count;        /* photonmapper "photonCount" (photons stored) */
    float photon_radius;          /* photonmapper "photonRadius" (0 in the XML:
                                     scene box diagonal / 500, photonmapper.cpp:55-56) */
    uint32_t num_images;          /* image textures and normal maps            */
    const nori_image_desc *images;
} nori_scene_desc;

/* ---- host-side scene loading (the plugin boundary) ----------------------- */
typedef struct nori_scene nori_scene;

/* Parse a Nori XML scene (same tags, `type` names, property names and
 * defaults as the reference).  width/height/spp > 0 override the XML. */
int nori_scene_load_xml(const char *path, int width, int height, int spp, nori_scene **out);
const nori_scene_desc *nori_scene_get_desc(const nori_scene *scene);
void nori_scene_free(nori_scene *scene);

/* Film border (ceil(radius - 0.5), block.cpp:57) and the 33-entry filter
 * table (block.cpp:59-64) for the scene's reconstruction filter. */
int nori_film_border(const nori_scene_desc *scene);
int nori_filter_table(const nori_scene_desc *scene, float table[NORI_FILTER_RESOLUTION + 1]);
/* RGBW film (H+2b)x(W+2b)x4 -> RGB bitmap HxWx3 divided by the filter weight
 * (ImageBlock::toBitmap, Color4f::divideByFilterWeight color.h:113-118). */
int nori_film_develop(const nori_scene_desc *scene, const float *rgbw, float *rgb);
/* Write an RGB float image as an uncompressed scanline OpenEXR file. */
int nori_write_exr(const char *path, const float *rgb, int width, int height);
/* Bitmap::saveToLDR (bitmap.cpp:109-139): sRGB transfer curve, x255 + 0.5,
 * clamp to [0, 255], 8-bit RGB PNG (zlib deflate, filter type 0). */
int nori_write_png(const char *path, const float *rgb, int width, int height);
/* Variance of each pixel's mean radiance from the statistics of
 * render_desc.variance_out (H x W x 8): out (H x W x 3) =
 * (sum L^2 - (sum L)^2 / n) / (n (n - 1)) per channel, in double precision;
 * 0 where n < 2.  The reference's own estimator (render.cpp:235-247,
 * 263-276: the spread of the running mean over the passes) does not estimate
 * the pixel variance; this one does (deviation D5). */
int nori_film_variance(const nori_scene_desc *scene, const float *stats, float *out);
/* The adaptive sampler's error metric (no reference counterpart: the
 * reference samples uniformly; deviation D11).  This is its one
 * statement; the device kernel (nori_gpu_block_error) computes the same.
 * Per pixel, from its 8 statistics floats (S1_c, S2_c for c = r, g, b, then n):
 *   n < 2: e_p = 0, otherwise
 *   m_c = S1_c / n,   v_c = max(0, S2_c - S1_c^2 / n) / (n (n - 1)),
 *   e_p = sqrt(v_r + v_g + v_b) / sqrt(m_r + m_g + m_b + 1e-3)
 * -- the standard error of the pixel mean relative to the square root of its
 * brightness.  Per 32x32 block: the block is tiled from its own origin into
 * 8x8 sub-tiles, each sub-tile's value is the mean of e_p over its pixels
 * inside the frame (a sub-tile wholly outside the frame does not exist), and
 * E_b is the MAXIMUM of the sub-tile means: one noisy corner (a caustic, a
 * light's edge) is not averaged away by 900 quiet pixels.
 * stats: H x W x 8 (render_desc.variance_out); errors: one float per frame
 * block, id = by*nbx + bx.  Host function, double precision. */
int nori_film_block_error(const nori_scene_desc *scene, const float *stats, float *errors);

/* NL-means denoiser <- denoiser/denoiser.py:53-66 on the GPU.  rgb: H x W x 3
 * image, variance: H x W per-pixel variance (the script's grey variance
 * image), out: H x W x 3.  radius = r (offsets in [-r, r]^2, <= 8), patch = f
 * (box filters of width 2(f-1)+1, 1 <= f <= 5), k = the script's k (0.02).
 * mode 0 reproduces the script's d2 (both variance terms 2 var(neighbour)),
 * mode 1 the textbook form (var_p + min(var_p, var_q), var_p + var_q).
 * Neighbours wrap around the image (np.roll), the box filters zero-pad
 * (convolve2d mode 'same').  Host buffers; runs on `device`. */
int nori_denoise(int device, const float *rgb, const float *variance, int width, int height, int radius,
                 int patch, float k, int mode, float *out);
/* First-hit features (nori_gpu_render_features): features (H x W x 8 sums) ->
 * out (H x W x 7): mean albedo (3), mean shading normal (3), mean depth (1) =
 * sum / count in double precision; a pixel with count 0 gives zeros; the
 * normal is the mean, NOT renormalised.  Host function. */
int nori_film_features(const nori_scene_desc *scene, const float *features, float *out);

/* Feature-guided NL-means denoiser (no reference counterpart: the reference's
 * script filters on colour alone; deviation D12).  This is its one
 * statement; nori_film_denoise_guided computes it on the host in double
 * precision, nori_denoise_guided on the GPU in fp32.
 *   rgb      H x W x 3 linear radiance I
 *   variance H x W     variance v of the pixel mean (the channels of
 *                      nori_film_variance summed)
 *   feat7    H x W x 7 nori_film_features: albedo a, normal n, depth z
 * Pixels outside the frame do not exist (no wrap-around, no zero fill).  For a
 * pixel p and every in-frame neighbour q = p + s, s in [-r, r]^2 (q = p included):
 *   d2c(p,q) = the mean, over the patch offsets o in [-f, f]^2 for which both
 *              p+o and q+o are inside the frame, of
 *              ( sum_c (I_c(p+o) - I_c(q+o))^2 - (v(p+o) + min(v(p+o), v(q+o))) )
 *              / ( eps + k^2 (v(p+o) + v(q+o)) )
 *   d2f(p,q) = |a_p - a_q|^2 / sigma_albedo^2 + |n_p - n_q|^2 / sigma_normal^2
 *              + ((z_p - z_q) / max(z_p, z_q, 1e-6))^2 / sigma_depth^2;
 *              a term whose sigma is +inf is exactly 0
 *   w(p,q)   = exp(-max(0, d2c)) exp(-d2f)
 *   out(p)   = sum_q w(p,q) I(q) / sum_q w(p,q) */
typedef struct nori_guided_desc {
    int32_t radius;      /* r: neighbours q = p + s, s in [-r, r]^2, 0 <= r <= 8          */
    int32_t patch;       /* f: patch offsets o in [-f, f]^2, 0 <= f <= 3                   */
    float   k;           /* colour distance scale (> 0)                                    */
    float   eps;         /* > 0                                                             */
    float   sigma_albedo, sigma_normal, sigma_depth;   /* > 0; +inf switches a term off     */
    uint32_t reserved;   /* must be 0 */
} nori_guided_desc;
/* NORI_ERR_INVALID (both): a null pointer, a non-positive size, radius or
 * patch out of range, a non-positive or NaN k, eps or sigma, reserved != 0. */
int nori_film_denoise_guided(const float *rgb, const float *variance, const float *feat7,
                             int width, int height, const nori_guided_desc *d, float *out);   /* host, fp64 */
/* Host buffers; runs on `device`.  Also NORI_ERR_INVALID (nothing launched)
 * when the tile staging of (radius, patch) exceeds the device's LDS per
 * work-group. */
int nori_denoise_guided(int device, const float *rgb, const float *variance, const float *feat7,
                        int width, int height, const nori_guided_desc *d, float *out);        /* GPU, host buffers */

/* Read the R, G, B planes of a scanline OpenEXR file (NONE/ZIPS/ZIP, HALF or
 * FLOAT) <- Bitmap::Bitmap (bitmap.cpp:23-80).  Call with rgb = NULL to get
 * the size, then with a buffer of 3*width*height floats (row-major). */
int nori_read_exr(const char *path, int *width, int *height, float *rgb);
/* Decode an image texture file as the reference's stbi_load(path, .., STBI_rgb)
 * does (stb_image v1.39: baseline JPEG, 8-bit PNG) <- ImageTexture / NormalMap
 * constructors (imagetexture.cpp:69-85, normalmap.cpp:69-85).  Call with
 * rgb = NULL to get the size, then with 3*width*height bytes (top row first). */
int nori_read_image(const char *path, int *width, int *height, uint8_t *rgb);

/* Host-side BVH build of the scene exactly as nori_gpu_create builds it (no
 * device needed) <- BVH::build + BVH::statistics (bvh.cpp:329-402): node count
 * and SAH cost of the reference-layout tree, device node count and depth, and
 * an FNV-1a hash of the leaf-order primitive ids. */
typedef struct nori_bvh_info {
    uint32_t ref_nodes;       /* nodes reachable in the reference layout      */
    uint32_t device_nodes;    /* 64-byte inner nodes of the device layout     */
    uint32_t depth;           /* inner-node depth of the device tree          */
    uint32_t num_prims;
    float sah_cost;           /* BVH::statistics cost of the root             */
    uint32_t pad;
    uint64_t order_hash;      /* FNV-1a over the leaf-order primitive ids     */
} nori_bvh_info;
int nori_scene_bvh_info(const nori_scene_desc *scene, nori_bvh_info *out);

/* Host-side scan list of a small scene (<= 64 primitives) exactly as
 * nori_gpu_create builds it (no device needed; introspection for tests -- no
 * reference counterpart): the primitive records in scan order (12 floats
 * each: v0 | prim id, e1 | sphere flag, e2 | leaf position; a sphere is
 * (centre | id, radius, ...)), per axis-plane pair the plane coordinate and
 * the in-plane filter of the binned extension kernel (8 floats: mid_B,
 * half_B + Kb, mid_C, half_C + Kb, Ka, c, 0, 0).  Call with null arrays for
 * the counts; records = 0 for a BVH scene. */
typedef struct nori_scan_info {
    uint32_t records;       /* 12-float records (pairs, other triangles padded, spheres) */
    uint32_t pairs;         /* axis-plane pairs: records 2g, 2g+1                          */
    uint32_t plane_end[3];  /* pairs of axis <= a                                          */
    uint32_t tris;          /* triangle records                                            */
} nori_scan_info;
int nori_scene_scan_list(const nori_scene_desc *scene, nori_scan_info *info, float *records, float *plane_c,
                         float *plane_f);

/* The bound of the fast body that both hipRTC programs below carry for this
 * scene: a wave whose rays all have |o_x| + |o_y| + |o_z| + |d_x| + |d_y| +
 * |d_z| <= *fast_max and mint > 0 scans the scene's literal records without
 * the per-test range checks and without the products whose record factor is
 * zero (same hits, t and primitive ids bit for bit; u, v equal as values);
 * every other wave takes the checked body.  0: the programs are built without
 * it -- a BVH scene, a scan list whose coordinates leave the bound no room, or
 * NORI_SCAN_FAST=0.  (Added without an ABI bump.) */
int nori_scene_scan_fast(const nori_scene_desc *scene, float *fast_max);

/* Compiles the scene's scan kernels specialised for its scan list (the
 * hipRTC program nori_gpu_create loads for scan-mode scenes, rtc.hip) for the
 * target `arch` (e.g. "gfx950"), without a device: *code_bytes = the code
 * object's size (0 for a BVH scene), *ms = the compile time (or cache read).
 * NORI_ERR_UNSUPPORTED when hipRTC is missing or the compile fails
 * (nori_gpu_last_error holds the log). */
int nori_scene_scan_rtc(const nori_scene_desc *scene, const char *arch, size_t *code_bytes, double *ms);

/* Compiles the scene's own shade kernel (the second hipRTC program of
 * nori_gpu_create, rtc.hip: the wavefront loop's k_shade for the scene's
 * integrator with the scan list as literals, so that the extension and shadow
 * scans inside it need no loads) for the target `arch`, without a device.
 * Only scan-mode scenes with the basic plugin set and a path integrator get
 * one: *code_bytes = 0 and *ms = 0 for every other scene, which the
 * library's ahead-of-time kernels serve.  Errors as nori_scene_scan_rtc.
 * (Added without an ABI bump, like the calls of the BVH rebuild.) */
int nori_scene_shade_rtc(const nori_scene_desc *scene, const char *arch, size_t *code_bytes, double *ms);

/* ---- GPU context ----------------------------------------------------------- */
typedef struct nori_gpu_ctx nori_gpu_ctx;

typedef struct nori_gpu_render_desc {
    uint32_t pass_begin;          /* first sample pass k                        */
    uint32_t pass_count;          /* passes to render (0 = scene spp)           */
    uint32_t num_blocks;          /* 0 = every 32x32 block of the frame         */
    const uint32_t *block_ids;    /* host array, id = by*nbx + bx (block.cpp:168) */
    uint64_t seed;                /* stream seed mixed into every sample id     */
    int32_t output_on_device;     /* rgbw_out is a device pointer on ctx device */
    uint32_t path_pool;           /* paths in flight (0 = default)              */
    int32_t timing;               /* nonzero: HIP events around every launch    */
    /* Optional per-pixel sample statistics, H x W x 8 floats ADDED into
     * (host or device memory like rgbw_out): sum of L (r, g, b), sum of L^2
     * (r, g, b), valid sample count, 0 -- of every valid sample in the pixel
     * it was taken in (unfiltered).  nori_film_variance turns them into the
     * variance of the pixel mean.  NULL: not collected. */
    float *variance_out;
} nori_gpu_render_desc;

typedef struct nori_gpu_stats {
    uint64_t samples;             /* camera samples completed                   */
    uint64_t invalid_samples;     /* NaN/Inf/negative radiance, dropped (block.cpp:94-98) */
    uint64_t rays_closest;        /* extension rays traced by k_extend          */
    uint64_t rays_shadow;         /* shadow rays traced (k_shadow, or k_shade itself) */
    uint64_t rays_finish;         /* rays traced inside the tail finisher       */
    uint64_t iterations;          /* wavefront iterations                       */
    uint64_t scene_bytes;         /* BVH nodes + primitive records in HBM       */
    uint32_t bvh_nodes, bvh_depth;
    uint32_t stream_parts;        /* pool parts on their own streams: each kernel
                                     runs stream_parts launches per iteration  */
    uint32_t path_pool;           /* paths in flight (the pool size used)     */
    double ms_total;              /* render wall time (host timer)              */
    /* with desc.timing: summed HIP-event time of each kernel, on the launch stream */
    double ms_extend, ms_shadow, ms_shade, ms_splat, ms_finish;
    /* scan-mode scenes: 1 when the context holds the scan kernels specialised
       for this scene (hipRTC at nori_gpu_create; the path integrators' trace
       launches and the trace API run them, the one-bounce integrators scan
       generically), the time that compile (or cache read) took then, and 1
       when its code object came from the cache */
    uint32_t scan_rtc, scan_rtc_cached;
    double ms_scan_rtc;
    /* 1 when the shade kernel traced its own next-event shadow rays instead of
       queueing them for k_shadow (scan-mode scenes with the basic plugins by
       default; NORI_NEE_INLINE=0/1 at nori_gpu_create), and 1 when it also
       traced each vertex's extension ray itself instead of reading the hit of
       a separate extension launch (the same scenes; NORI_EXT_INLINE=0/1) */
    uint32_t nee_inline, ext_inline;
} nori_gpu_stats;

typedef struct nori_gpu_hit {
    float t;                      /* +inf on miss                               */
    int32_t prim;                 /* global primitive id (shape order), -1 miss */
    float u, v;                   /* barycentrics (mesh)                        */
} nori_gpu_hit;

const char *nori_gpu_last_error(void);
int nori_gpu_abi_version(void);
int nori_gpu_device_count(int *count);
int nori_gpu_create(const nori_scene_desc *scene, int device, nori_gpu_ctx **out);
/* Render passes [pass_begin, pass_begin+pass_count) of the given blocks and
 * ADD the filtered samples into rgbw_out ((H+2b)x(W+2b)x4 floats, caller
 * owned, host or device memory).  Blocking. */
int nori_gpu_render(nori_gpu_ctx *ctx, const nori_gpu_render_desc *desc,
                    float *rgbw_out, nori_gpu_stats *stats);
/* nori_film_block_error on the context's device: stats is H x W x 8 floats in
 * host memory, or (stats_on_device != 0) in device memory on the context's
 * device, 16-byte aligned; errors is a HOST array of one float per frame
 * block.  The difference S2 - S1^2/n is taken in fp64, the rest in fp32: the
 * result agrees with the host function to fp32 rounding.  Blocking. */
int nori_gpu_block_error(nori_gpu_ctx *ctx, const float *stats, int stats_on_device, float *errors);

/* Adaptive sampling: blocks whose error metric E_b (nori_film_block_error)
 * has fallen to `threshold` stop early; the others go on to the cap. */
typedef struct nori_gpu_adaptive_desc {
    uint32_t min_passes;     /* first round, >= 2 */
    uint32_t max_passes;     /* per-block cap; 0 = scene sampleCount */
    float    threshold;      /* a block stops once E_b <= threshold */
    uint32_t reserved;       /* must be 0; pads passes_out to 8 bytes */
    uint32_t *passes_out;    /* host, one per frame block: passes rendered (0 = block not selected); may be NULL */
    float    *error_out;     /* host, one per frame block: E_b of the final statistics; may be NULL */
} nori_gpu_adaptive_desc;
/* Renders in rounds.  Round 0 renders passes [pass_begin, pass_begin +
 * min_passes) of every selected block.  After each round E_b of the blocks
 * just rendered is evaluated on the device; a block stays active while
 * E_b > threshold and its pass count is below the cap, and the next round
 * renders as many passes again as the active blocks have had, clamped to the
 * cap (counts min, 2 min, 4 min, ..., max), continuing their pass numbering.
 * So block b receives exactly the samples of passes [pass_begin, pass_begin +
 * passes_out[b]): the film equals plain nori_gpu_render calls with those
 * counts.  E_b is evaluated after the last round too.
 * From `desc`: pass_begin, seed, num_blocks / block_ids, output_on_device,
 * path_pool, timing and variance_out keep their nori_gpu_render meaning
 * (film and statistics are ADDED into the caller's buffers, once, at the
 * end); pass_count is ignored.  The metric is that of this call's samples:
 * statistics are collected on the device whether or not variance_out is set.
 * stats: samples, invalid_samples, the ray counters, iterations and the ms_*
 * kernel times are summed over the rounds; ms_total is the wall time of the
 * call.  nori_gpu_cancel is honoured between and within rounds
 * (NORI_ERR_CANCELLED; nothing is added to host buffers then), and
 * nori_gpu_progress rises over the whole call as samples done over the upper
 * bound cap x selected pixels.  NORI_ERR_INVALID: min_passes < 2, a cap below
 * min_passes, a negative or NaN threshold (+inf is valid: one round),
 * reserved != 0.  Works for the wavefront and the one-bounce integrators.
 * There is no sharded form: per-pixel statistics are not summed across ranks
 * (nori_gpu_render_sharded); callers who drive rounds over several GPUs sum
 * the statistics themselves and use nori_film_block_error. */
int nori_gpu_render_adaptive(nori_gpu_ctx *ctx, const nori_gpu_render_desc *desc,
                             const nori_gpu_adaptive_desc *ad, float *rgbw_out, nori_gpu_stats *stats);
/* First-hit features of the camera samples of passes [pass_begin, pass_begin+pass_count)
 * of the selected blocks, ADDED into `features` (H x W x 8 floats, host or device memory
 * as desc->output_on_device says; 16-byte aligned on the device):
 *   0..2 albedo (sum)   3..5 world-space shading normal, signed (sum)
 *   6    hit distance t along the primary ray (sum)   7 camera samples taken (count)
 * Sample (pass k, pixel) draws from the renderer's own stream of that sample
 * (jitter, then aperture sample), so its primary ray is the render's, for
 * every camera; with chromatic aberration the features follow the green
 * channel's ray.  Hit: the normal is the shading normal (normal-mapped where
 * the mesh has a map: the vector the `normals` integrator returns before its
 * fabs), the depth is t, the albedo is by BSDF: diffuse -- the albedo texture
 * at the hit's uv; microfacet -- kd; disney -- base_color; mirror and
 * dielectric -- (1, 1, 1).  Emission plays no part.  Miss: only the count
 * rises, so a missed sample is recognisable by its zero normal.
 * Each pixel's eight values are read, the samples added in pass order and the
 * sums written back: no atomics, so the result is bitwise reproducible and a
 * pass range split over several calls gives the identical buffer.  Works on a
 * context of any integrator (no path pool).  From `desc`: pass_count 0 = the
 * scene's sampleCount; path_pool is ignored; timing: the kernel time in
 * stats->ms_shade; variance_out must be NULL (NORI_ERR_INVALID otherwise).
 * stats: samples, rays_closest (one per sample), ms_total.  nori_gpu_cancel is
 * honoured between chunks of passes (NORI_ERR_CANCELLED; a host buffer is left
 * unchanged then) and nori_gpu_progress rises over the call.  Blocking. */
int nori_gpu_render_features(nori_gpu_ctx *ctx, const nori_gpu_render_desc *desc,
                             float *features, nori_gpu_stats *stats);
/* Trace n rays (host arrays; ray = o.xyz, mint, d.xyz, maxt) with the
 * reference's BVH semantics: closest hit, or any hit when any_hit != 0. */
int nori_gpu_trace(nori_gpu_ctx *ctx, const float *rays, uint32_t n, int any_hit,
                   nori_gpu_hit *hits);

/* ---- ray queries with full hit records ------------------------------------
 * Scene::rayIntersect(ray, its) + setHitInformation: one 64-byte record = four float4. */
typedef struct nori_gpu_surface {
    float p[3];   float t;        /* its.p ; its.t, +inf on a miss                         */
    float ng[3];  int32_t prim;   /* its.geoFrame.n ; global primitive id, -1 on a miss    */
    float ns[3];  int32_t shape;  /* its.shFrame.n (normal-mapped) ; shape index, -1 miss  */
    float uv[2];  float bary[2];  /* its.uv after setHitInformation ; nori_gpu_hit's u, v   */
} nori_gpu_surface;

typedef struct nori_gpu_query_desc {
    uint32_t n;          /* rays */
    int32_t  any_hit;    /* as nori_gpu_trace; only with hits, surf must be NULL */
    int32_t  on_device;  /* rays / hits / surf are device pointers on the context's device, 16-byte aligned */
    uint32_t reserved;   /* must be 0 */
} nori_gpu_query_desc;

/* The record of hit i of ray i (8 floats: o.xyz, mint, d.xyz, maxt), on the
 * host in fp32 with the kernels' operation order (no device needed).  This is
 * the record's one statement; the device kernel (nori_gpu_query) computes the same.
 *   bary, t, prim: the nori_gpu_hit values verbatim; shape: the shape that
 *   owns primitive `prim` (primitives are numbered in shape order, a mesh
 *   takes tri_count ids, a sphere one).
 *   Mesh (vertices p0, p1, p2 of triangle prim, b = 1 - (u + v)):
 *     p  = (b p0 + u p1) + v p2
 *     ng = normalize(cross(p1 - p0, p2 - p0))
 *     uv = (b uv0 + u uv1) + v uv2; the barycentrics (u, v) if the mesh has no uvs
 *     ns = normalize((b n0 + u n1) + v n2); with a normal map (meshes with
 *          normals only) the texel at uv (x = (int)(uv.x W), y = (int)(uv.y H),
 *          wrapped or clamped as the image says), m = normalize(2 byte / 255 - 1)
 *          per channel, taken from the frame of the interpolated normal
 *          (Frame(n), common.cpp:274-283) to the world: ns = s m.x + t m.y + n m.z,
 *          NOT renormalised (NormalMap::eval, mesh.cpp:147-155);
 *          ns = ng if the mesh has no normals
 *   Sphere (centre c): p = o + t d, ng = ns = normalize(p - c),
 *     uv = (0.5 + acos(n.z) / (2 pi), phi / pi), phi = atan2(n.y, n.x) wrapped
 *     to [0, 2 pi) (sphericalCoordinates, common.cpp:264-272) -- always
 *     computed, whatever the BSDF
 *   Miss (prim < 0): t = +inf, prim = shape = -1, every other float 0.
 * NORI_ERR_INVALID: a null pointer, a primitive id outside the scene. */
int nori_scene_surface(const nori_scene_desc *scene, uint32_t n, const float *rays,
                       const nori_gpu_hit *hits, nori_gpu_surface *out);

/* The record's adjoint in the mesh vertices, on the host (no device needed):
 * for a gradient grad_surf[i] of some scalar in record i (the record's own
 * layout, so an (n, 16) float gradient of a record array passes through
 * unchanged), what that scalar's gradient in the vertex positions and vertex
 * normals receives from hit i.  This is the one statement; the device call
 * (nori_gpu_surface_grad) forms the same terms and adds them in any order.
 *   positions, normals: num_vertices x 3 floats each, the geometry the record
 *     is differentiated at; NULL: the scene's own arrays.
 *   Of grad_surf[i] only p, t, ng and ns are read (g_p, g_t, g_ng, g_ns); the
 *     words at prim, shape, uv and bary are ignored and may hold anything (NaN
 *     bit patterns included): uv and bary have no gradient, texture
 *     coordinates are not vertices that nori_gpu_update_vertices moves.
 *   What is held fixed: the hit set (prim), the barycentrics (u, v) for p and
 *     ns, the ray (o, d) for t.  So g_p is the derivative of the material
 *     point at fixed barycentrics; a caller who wants the point where the
 *     fixed ray meets the moving triangle (p = o + t d) adds d . g_p to g_t
 *     and passes g_p = 0.  t is differentiated as the exact function
 *     t = N.(p0 - o) / (N.d) whose fp32 value the tracer returns.
 * Hit i: prim, u, v, t from hits[i]; o = rays[8i .. 8i+2], d = rays[8i+4 ..
 * 8i+6]; vertices p0, p1, p2 and vertex normals n0, n1, n2 of triangle prim
 * (vertex ids f0, f1, f2).  Every operation is fp32, unfused, in this order
 * (dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; cross as usual, each component
 * one subtraction of two products; vectors componentwise):
 *     b   = 1 - (u + v)
 *     e1  = p1 - p0;  e2 = p2 - p0;  N = cross(e1, e2)
 *     len = sqrt(dot(N, N));  D = dot(N, d)
 *     len > 0 and D != 0, else the hit contributes nothing
 *     ng  = N / len
 *     g'  = g_ng on a mesh with vertex normals, g_ng + g_ns on one without (ns = ng there)
 *     gN  = (g' - ng * dot(ng, g')) / len
 *     s   = g_t / D;  ph = o + d * t
 *     gN  = gN + (p0 - ph) * s
 *     ge1 = cross(e2, gN);  ge2 = cross(gN, e1)
 *     g_p0 = (g_p * b + N * s) - (ge1 + ge2)
 *     g_p1 = g_p * u + ge1
 *     g_p2 = g_p * v + ge2
 *   and, on a mesh with vertex normals and no normal map,
 *     M   = (n0 * b + n1 * u) + n2 * v;  lm = sqrt(dot(M, M))
 *     lm > 0, else g_n0 = g_n1 = g_n2 = 0 (the position terms stay)
 *     ns  = M / lm
 *     gM  = (g_ns - ns * dot(ns, g_ns)) / lm
 *     g_n0 = gM * b;  g_n1 = gM * u;  g_n2 = gM * v
 *   On a normal-mapped shape g_ns contributes nothing, to positions or normals:
 *   the frame built around the interpolated normal is piecewise (Frame(n)
 *   branches on the normal's components) and the mapped normal is not
 *   renormalised, so that derivative is left out; g_p, g_t and g_ng still count.
 *   A miss (prim < 0) and a sphere hit contribute nothing.
 * terms (NULL, or n x 18 floats): g_p0, g_p1, g_p2, g_n0, g_n1, g_n2 of hit i
 * at terms[18 i], zeros where the hit contributes nothing or the mesh has no
 * normal terms.
 * The sums: grad_positions[3 f0 ..] receives g_p0, [3 f1 ..] g_p1, [3 f2 ..]
 * g_p2 (grad_normals likewise; NULL: the normal terms are not formed and the
 * positions' result is the same bits).  Each destination float is accumulated
 * in float64 over the hits in order and the sum is added once, in float64, to
 * the value already there and rounded to fp32; a destination that receives no
 * term is not touched.
 * NORI_ERR_INVALID, nothing written: a null scene, rays, hits, grad_surf or
 * grad_positions; a primitive id outside the scene; a non-finite position or
 * normal (of the arrays in use). */
int nori_scene_surface_grad(const nori_scene_desc *scene, const float *positions, const float *normals,
                            uint32_t n, const float *rays, const nori_gpu_hit *hits,
                            const nori_gpu_surface *grad_surf, float *grad_positions, float *grad_normals,
                            float *terms);

/* Trace desc->n rays as nori_gpu_trace does (the same kernels: `hits` is
 * bit-identical to its result) and, with `surf`, fill the record of every
 * closest hit (nori_scene_surface).  hits and surf may each be NULL, not both.
 * on_device: the three pointers are device memory on the context's device,
 * nothing is copied and nothing allocated per call (a context-owned hit
 * buffer serves hits == NULL); the caller has made the rays ready before the
 * call, as with nori_gpu_render's device film.  Otherwise they are host
 * arrays, staged through context-owned device buffers that later calls reuse,
 * in chunks of at most NORI_QUERY_CHUNK rays (environment, default 4194304).
 * Blocking; runs on the context's stream: concurrent use with a render (or
 * another query) on the same context is not supported.
 * NORI_ERR_INVALID, nothing launched: a null ctx, desc or rays; both outputs
 * null; any_hit with surf; reserved != 0; on_device with a pointer that is
 * not 16-byte aligned.  n == 0 is a no-op.
 * stats (may be NULL): rays_closest or rays_shadow (any_hit) = n, ms_total
 * (wall time), ms_extend / ms_shade = HIP-event time of the trace / record kernels. */
int nori_gpu_query(nori_gpu_ctx *ctx, const nori_gpu_query_desc *desc, const float *rays,
                   nori_gpu_hit *hits, nori_gpu_surface *surf, nori_gpu_stats *stats);

/* nori_scene_surface_grad on the device, for the vertices the context holds
 * now (as nori_gpu_create loaded them or nori_gpu_update_vertices last set
 * them; the tree plays no part, so nori_gpu_rebuild_bvh changes nothing).  The
 * kernel forms the statement's fp32 terms bit for bit and ADDS them into
 * grad_positions and, unless NULL, grad_normals (num_vertices x 3 floats each)
 * with float atomics, after summing on chip the terms of a work-group's hits
 * on the same triangle: the order of the additions is not fixed, so a sum of
 * several terms agrees with the statement's to fp32 rounding of its partial
 * sums, not bit for bit (a destination with one term does).
 * on_device: rays, hits, grad_surf (16-byte aligned) and the two outputs
 * (4-byte aligned) are device memory on the context's device, used in place;
 * nothing is allocated per call.  Otherwise they are host arrays: the inputs
 * pass through the context's staging buffers in chunks of at most
 * NORI_QUERY_CHUNK hits, the sums are formed in zeroed device buffers and added
 * to the caller's arrays once at the end.  Works on a context of any
 * integrator and either traversal mode.  Blocking, on the context's stream.
 * A primitive id outside the scene contributes nothing (the kernel cannot
 * refuse).  n == 0 is a no-op.
 * NORI_ERR_INVALID, nothing launched and nothing written: a null ctx, desc,
 * rays, hits, grad_surf or grad_positions; reserved != 0; on_device with a
 * misaligned pointer or one that is not device memory.
 * stats (may be NULL): ms_total (wall time), ms_shade = HIP-event time of the kernel. */
typedef struct nori_gpu_surface_grad_desc {
    uint32_t n;            /* hits */
    int32_t  on_device;    /* all five arrays are device pointers on the context's device */
    uint32_t reserved[2];  /* must be 0 */
} nori_gpu_surface_grad_desc;
int nori_gpu_surface_grad(nori_gpu_ctx *ctx, const nori_gpu_surface_grad_desc *desc, const float *rays,
                          const nori_gpu_hit *hits, const nori_gpu_surface *grad_surf,
                          float *grad_positions, float *grad_normals, nori_gpu_stats *stats);

/* Camera::sampleRay for the renderer's own samples: the primary ray of sample
 * (pass pass_begin + k, pixel pix = y W + x) at rays[8 (k H W + pix)] (o.xyz,
 * mint, d.xyz, maxt), for k < pass_count and the pixels of the selected blocks
 * (other entries are left untouched).  The sample draws from
 * wave_seed(seed, (pass_begin + k) W H + pix): the jitter first, then the
 * aperture sample -- what the integrators and nori_gpu_render_features do;
 * with chromatic aberration it is the green channel's ray.  From `desc`:
 * pass_begin, pass_count (0 = the scene's sampleCount), seed, num_blocks /
 * block_ids and output_on_device (rays is device memory, 16-byte aligned);
 * the other fields are ignored, variance_out must be NULL (NORI_ERR_INVALID).
 * rays: pass_count x H x W x 8 floats.  Works on a context of any integrator.
 * Blocking, on the context's stream. */
int nori_gpu_camera_rays(nori_gpu_ctx *ctx, const nori_gpu_render_desc *desc, float *rays);

/* ---- shading queries: the renderer's BSDFs, emitters and random numbers ----
 * (no reference counterpart: its BSDFs and emitters are virtuals called from
 * Li; deviation D16).  With nori_gpu_camera_rays and nori_gpu_query
 * they are what an integrator written outside the library needs to reproduce
 * the built-in ones sample for sample.  They trace nothing, so they work on a
 * context of any integrator and traversal mode, and after
 * nori_gpu_update_vertices / nori_gpu_rebuild_bvh they answer for the geometry
 * as it is now (the lights' area tables included).  Blocking, on the context's
 * stream, like nori_gpu_query. */
typedef struct nori_gpu_shading_desc {
    uint32_t n;          /* elements */
    int32_t  on_device;  /* every array is device memory on the context's device */
    int32_t  emitter;    /* nori_gpu_emitter_sample only: the emitter for every element when ids == NULL */
    uint32_t reserved;   /* must be 0 */
} nori_gpu_shading_desc;
/* Common to the four calls below.
 * Arrays.  surf: n records as nori_gpu_query writes them (64 bytes each; 16-byte
 * aligned on the device).  Directions and points (wi, wo, x, from): n x 3
 * floats, packed, world space; u: n x 2 floats; ids: n int32 -- each 4-byte
 * aligned on the device.  out: n rows of 8, 8, 12 and 4 floats, 16-byte aligned
 * on the device.  on_device: used in place, nothing copied and nothing
 * allocated per call, the caller has made the inputs ready.  Otherwise host
 * arrays, staged through context-owned buffers in chunks of at most
 * NORI_QUERY_CHUNK elements.
 * Of a record only ns, shape and uv are read (nori_gpu_emitter_eval: p, ns and
 * shape).  Its shading frame is Frame(ns) (frame.h:49-51, coordinateSystem
 * common.cpp:274-283): n = ns as stored (not renormalised); if |n.x| > |n.y|
 * t = (n.z, 0, -n.x) / sqrt(n.x n.x + n.z n.z), else t = (0, n.z, -n.y) /
 * sqrt(n.y n.y + n.z n.z), the division done as a multiplication by the
 * correctly rounded reciprocal; s = cross(t, n).  That is the render's own
 * frame at that hit bit for bit (spheres, meshes with and without normals,
 * normal-mapped meshes).  to_local(v) = (dot(v, s), dot(v, t), dot(v, n)) with
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; to_world(v) = (s v.x + t v.y) + n v.z.
 * The BSDF is that of shape `shape`, textures are looked up at the record's uv;
 * for an image texture a uv coordinate that is NaN or beyond +-2^30 / max(W, H)
 * of the image counts as 0 (so that no texel index can leave its image).
 * A record whose shape is < 0 or >= the scene's num_shapes is a miss: every
 * output float of that element is 0 (nori_gpu_query writes shape -1).
 * NORI_ERR_INVALID, nothing launched: a null ctx, desc or array (ids excepted);
 * reserved != 0; on_device with a pointer that is misaligned or that the HIP
 * runtime does not know as device memory; with host arrays a record whose
 * shape is < -1 or >= num_shapes, or an emitter id (in ids, or desc->emitter
 * when ids == NULL) outside [0, num_emitters).  With device arrays the
 * kernels' own range guards apply to records, ids and desc->emitter alike
 * (zeros, as stated).  n == 0 is a no-op.
 * Every refusal leaves the context usable. */

/* BSDF::eval and BSDF::pdf at each record.  wi: away from the surface towards
 * where the path came from (minus the incoming ray's direction); wo: the other
 * direction.  Both are taken to the shading frame with to_local, the measure
 * is the solid angle.  out row: eval r, g, b (no cosine factor), pdf,
 * wo_local.z, wi_local.z, 0, 0 -- the cosines so that a caller forms f * cos
 * with the renderer's own to_local.  (The `direct` integrator alone calls its
 * BSDF with the two directions swapped.) */
int nori_gpu_bsdf_eval(nori_gpu_ctx *ctx, const nori_gpu_shading_desc *desc, const nori_gpu_surface *surf,
                       const float *wi, const float *wo, float *out);
/* BSDF::sample at each record with the 2D sample u (x drawn first): the local
 * wi as above, then out row: to_world(sampled wo) x, y, z; BSDF::pdf of the
 * sampled pair (what direct_mis and path_mis weigh the BSDF sample with; 0
 * for the discrete lobes); the sample weight r, g, b (eval * cos / pdf, what
 * BSDF::sample returns); the measure as a float (1 solid angle, 2 discrete).
 * A zero weight gives an all-zero row: the renderer ends the path there
 * without a ray (deviation D1), so there is no direction to report.  The next
 * ray of the renderer is (p, NORI_EPSILON, direction, +inf). */
int nori_gpu_bsdf_sample(nori_gpu_ctx *ctx, const nori_gpu_shading_desc *desc, const nori_gpu_surface *surf,
                         const float *wi, const float *u, float *out);
/* Emitter::sample of emitter ids[i] (or desc->emitter for every element when
 * ids is NULL) from the reference point x[i] with the 2D sample u[i].
 * out row: wi x, y, z (unit, from x towards the light); the shadow ray's maxt;
 * radiance * attenuation / pdf r, g, b -- NOT scaled by the emitter count;
 * pdf_em (area light: the area-measure density 1 / area when the sampled
 * point faces x, else 0, with a zero radiance; point and spot: 1;
 * environment map: its solid-angle density); the sampled point p x, y, z; 0.
 * The renderer's shadow ray is (x, NORI_EPSILON, wi, maxt): trace it with
 * nori_gpu_query(any_hit) and drop the sample if it hits.  The direct_*
 * integrators sample every emitter in index order with one next2D each; the
 * path integrators pick one, li = min(floor(N * ul), N - 1) for a draw ul
 * taken before the 2D sample, and use Li * N (N = num_emitters).
 * Area lights: mesh -- triangle by the area CDF with sample reuse, then
 * squareToUniformTriangle, normal interpolated or geometric; sphere --
 * c + r * squareToUniformSphere(u).  wi = normalize(p - x), attenuation =
 * dot(n, -wi) / |p - x|^2, maxt = |p - x| - NORI_EPSILON.  Point / spot:
 * power (times the spot falloff) / (4 pi |p - x|^2).  Environment map: as the
 * renderer samples it (deviation D4), maxt = 100000; a sample outside [0, 1)
 * is taken at the nearest table row. */
int nori_gpu_emitter_sample(nori_gpu_ctx *ctx, const nori_gpu_shading_desc *desc, const int32_t *ids,
                            const float *x, const float *u, float *out);
/* What the emitter of the hit shape radiates towards `from`, and the density
 * with which nori_gpu_emitter_sample would have produced that hit: both at the
 * record's ns and wi = normalize(p - from) (EmitterQueryRecord(from, p, ns)).
 * out row: Emitter::eval r, g, b; Emitter::pdf (the pdf_em of
 * nori_gpu_emitter_sample: bit-equal for the same point and direction).  Area
 * light: radiance and 1 / area when dot(ns, -wi) > 0, else zeros; environment
 * map: its value and density along wi.  A shape without an emitter gives zeros.
 * This is the emission term of every integrator at a hit seen from the ray's
 * origin, and the emitter side of the BSDF-sampling weight of direct_mis /
 * path_mis: w_mat = pdf_mat / (pdf_mat + pdf_em) if the sum is > 0. */
int nori_gpu_emitter_eval(nori_gpu_ctx *ctx, const nori_gpu_shading_desc *desc, const nori_gpu_surface *surf,
                          const float *from, float *out);

/* ---- differentiable materials ---------------------------------------------
 * The material row: NORI_MATERIAL_FLOATS floats per entry of the scene's
 * bsdfs[], in its order -- the parameters that may change under a context and
 * that nori_gpu_bsdf_eval is differentiated in.
 *   words 0-2    the colour: diffuse albedo (constant_color, or the
 *                checkerboard's value1) / microfacet kd / disney base_color
 *   word  3      microfacet alpha
 *   words 4-9    disney metallic, specular, roughness, sheen, sheen_tint, specular_tint
 *   words 10-12  checkerboard value2
 *   words 13-15  reserved: ignored when set, 0 when read, 0 in every gradient
 * The words in use: diffuse with a constant albedo 0-2, with a checkerboard
 * 0-2 and 10-12, with an image texture none; microfacet 0-3; disney 0-2 and
 * 4-9; mirror and dielectric none.  A word that the BSDF's type does not use
 * is ignored when set (it may hold anything, NaN included), reads 0 and is 0
 * in every gradient.  Held: the IORs, the checkerboard's delta and scale,
 * image texels, normal maps, emitters. */
#define NORI_MATERIAL_FLOATS 16

/* The rows of the scene as loaded: rows[16 b ..] for b < num_bsdfs.  Host only.
 * NORI_ERR_INVALID: a null argument. */
int nori_scene_materials(const nori_scene_desc *scene, float *rows);

/* nori_gpu_bsdf_eval's adjoint in the material rows, on the host (no device
 * needed): for a gradient grad_out[i] of some scalar in output row i of
 * nori_gpu_bsdf_eval(surf, wi, wo) (its own layout, n x 8 floats), what that
 * scalar's gradient in the rows receives from element i.  This is the one
 * statement; nori_gpu_bsdf_grad forms the same terms on the device.
 *   materials: num_bsdfs x 16 floats, the rows to differentiate at (the derived
 *     constants ks and disney's pdf alpha follow them as in
 *     nori_gpu_update_materials); NULL: the scene's own.
 *   Of grad_out[i] words 0-2 (g_r, g_g, g_b: the gradient in eval) and word 3
 *     (g_p: in pdf) are read; words 4-7 are never read and may hold anything:
 *     the cosines do not depend on the parameters.
 *   Held: surf, wi, wo (no gradient in them), the IORs, textures' layout.
 * Element i: the frame, to_local, the uv rule and the miss rule are
 * nori_gpu_bsdf_eval's; b is the BSDF of the record's shape; wi, wo below are
 * local.  Every operation is fp32, rounded once, in the order written (sums
 * and products left to right; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
 * ipi = 1/pi as a float), the forward factors D, F, G1, tan, schlick, ggx,
 * gtr2 are the routines bsdf_eval itself calls, and a branch of eval (of pdf)
 * that returns zero gives zero terms for g_r, g_g, g_b (for g_p).
 *   diffuse, constant:  eval is zero unless wi.z > 0 and wo.z > 0; then
 *       t[c] = g_c * ipi, c = 0, 1, 2.  pdf has no parameter.
 *   diffuse, checkerboard: the same three products, at words 0-2 in a cell of
 *       value1 and at words 10-12 in a cell of value2 (the forward's parity).
 *   diffuse with an image texture, mirror, dielectric, a miss: a zero row.
 *   microfacet: h = normalize(wi + wo), D = beckmann_D(h), F = fresnel(h.wi),
 *       Gi = smith_G1(wi, h), Go = smith_G1(wo, h), den = 4 wi.z wo.z, gs = (g_r + g_g) + g_b
 *       tt = tan_theta(h) / alpha;  dD = D * (2 * (tt * tt - 1) / alpha)
 *       dG1(v): 0 where smith_G1 returns early (tan_theta(v) == 0, the sign
 *         test) or a >= 1.6, a = 1 / (alpha tan_theta(v)); else with
 *         N = 3.535 a + 2.181 a a, Q = 1 + 2.276 a + 2.577 a a:
 *         ((3.535 + 4.362 a) * Q - N * (2.276 + 5.154 a)) / (Q * Q) * (-(a / alpha))
 *       dG = dG1(wi) * Go + Gi * dG1(wo)
 *       s_ks = D * F * (Gi * Go) / den                      (d eval / d ks)
 *       s_al = ks * F * (dD * (Gi * Go) + D * dG) / den     (d eval / d alpha)
 *       pdf is zero unless wo.z > 0; then J = h.z / (4 |h.wo|),
 *       p_ks = D * J - wo.z * ipi,  p_al = ks * (dD * J);   else p_ks = p_al = 0
 *       t[c] = g_c * ipi;  t[3] = gs * s_al + g_p * p_al
 *       ks = 1 - max(kd): t[m] = t[m] - (gs * s_ks + g_p * p_ks) for the first
 *       channel m that attains the maximum.  F has no term (the IORs are held).
 *   disney: eval is zero unless wi.z >= 0 and wo.z >= 0; the adjoint of
 *       disney.cpp's expression written out in csrc/bsdf_grad.h, with these
 *       conventions: alpha = max(0.001, r r) has derivative 2 r where
 *       r r > 0.001 and 0 elsewhere (the eval's float square and the pdf's
 *       double square each by its own comparison); ctint = base / l carries
 *       the derivative through l = luminance(base) where l > 0, else none;
 *       fd90's roughness term counts; gtr2's zero branch has derivative 0.
 *       pdf is zero unless wo.z > 0.
 *   A row in which any float comes out non-finite, or whose g_r, g_g, g_b or
 *   g_p is non-finite, is replaced by zeros as a whole (den = 0 at grazing
 *   directions, an overflowing lobe): one bad sample does not poison a sum.
 * terms (NULL, or n x 16 floats): the row of element i at terms[16 i].
 * The sums: grad_materials[16 b + w] receives word w of every element on BSDF
 * b, accumulated in float64 in element order and added once, in float64, to
 * the value already there and rounded to fp32; a destination that receives no
 * non-zero term is not touched.
 * NORI_ERR_INVALID, nothing written: a null scene, surf, wi, wo, grad_out or
 * grad_materials; a record whose shape is < -1 or >= num_shapes. */
int nori_scene_bsdf_grad(const nori_scene_desc *scene, const float *materials, uint32_t n,
                         const nori_gpu_surface *surf, const float *wi, const float *wo, const float *grad_out,
                         float *grad_materials, float *terms);

/* Set every BSDF's parameter words from `rows` (num_bsdfs x 16 floats, host
 * memory, or device memory used in place when on_device: 4-byte aligned) and
 * recompute the derived constants (microfacet ks = 1 - max(kd), disney's pdf
 * alpha = max(1e-3, r r) squared in double) with nori_gpu_create's own
 * operations.  Both copies of the BSDF table are updated (the small-scene
 * blob's too), so every later render, li, feature pass and shading query sees
 * the new values, bit-identical to a context created from a scene loaded with
 * them.  No plan decision and no scene-specialised kernel depends on a
 * parameter value (only on BSDF types and texture kinds, which are held), so
 * this works in either traversal mode.  Blocking, on the context's stream.
 * Refused with nothing changed -- NORI_ERR_INVALID: a null argument, num_bsdfs
 * other than the scene's, reserved != 0, on_device with a misaligned pointer
 * or one that is not device memory, a non-finite float in a word in use
 * (counted on the device in a pass of its own before anything is modified);
 * NORI_ERR_UNSUPPORTED: a photonmapper context (its map was traced at
 * creation).  Every success bumps the context's materials version. */
typedef struct nori_gpu_materials_desc {
    uint32_t num_bsdfs;    /* must equal the scene's */
    int32_t  on_device;    /* rows is a device pointer on the context's device */
    uint32_t reserved[2];  /* must be 0 */
} nori_gpu_materials_desc;
int nori_gpu_update_materials(nori_gpu_ctx *ctx, const nori_gpu_materials_desc *desc, const float *rows);
/* The rows the context holds now (host array, num_bsdfs x 16; may be NULL) and
 * the number of successful nori_gpu_update_materials calls so far (may be NULL). */
int nori_gpu_materials(nori_gpu_ctx *ctx, float *rows, uint64_t *version);

/* nori_scene_bsdf_grad on the device, for the materials the context holds now.
 * The kernel forms the statement's terms (bit for bit where the forward has
 * no transcendental: diffuse, checkerboard, disney; microfacet to the device
 * library's expf) and ADDS their sums into grad_materials (num_bsdfs x 16).
 * Reproducible: up to NORI_BSDF_GRAD_MAX_TABLE BSDFs the sums are formed
 * without atomics -- per wave in a fixed order, per work-group in wave order
 * into one slab of partial sums, the slabs in slab order by a second kernel,
 * which adds each destination once -- so the same inputs give the same bits on
 * every call, whatever the device's scheduling.  (A destination's value is
 * the fp32 sum of its terms in that fixed tree, within m 2^-24 A of the
 * statement's for m terms of magnitude sum A.)  With more BSDFs, or with
 * NORI_BSDF_GRAD_TABLE=0 in the environment, the sums of a wave's elements on
 * one BSDF are added with float atomics: their order is not fixed, and neither
 * are the last bits.
 * on_device: surf, grad_out, grad_materials, terms (16-byte aligned) and wi,
 * wo (4-byte aligned) are device memory used in place.  Otherwise host arrays,
 * staged through context buffers in chunks of whole tiles of 256 elements, at
 * most NORI_QUERY_CHUNK elements (at least one tile); the chunks continue one
 * set of partial sums, so the chunking does not show in the bits; the sums are
 * formed in a zeroed device buffer and added to the caller's array once at
 * the end.  Nothing is allocated per call once the
 * context's buffers have grown to the call's size.  terms may be NULL.  Works
 * on a context of any integrator and either traversal mode.  Blocking, on the
 * context's stream.  n == 0 is a no-op.
 * NORI_ERR_INVALID, nothing launched and nothing written: a null ctx, desc,
 * surf, wi, wo, grad_out or grad_materials; reserved != 0; on_device with a
 * misaligned pointer or one that is not device memory; host records with a
 * shape < -1 or >= num_shapes (device records: such an element adds nothing).
 * stats (may be NULL): ms_total (wall time), ms_shade = HIP-event time of the kernels. */
#define NORI_BSDF_GRAD_MAX_TABLE 64
typedef struct nori_gpu_bsdf_grad_desc {
    uint32_t n;            /* elements */
    int32_t  on_device;    /* every array is a device pointer on the context's device */
    uint32_t reserved[2];  /* must be 0 */
} nori_gpu_bsdf_grad_desc;
int nori_gpu_bsdf_grad(nori_gpu_ctx *ctx, const nori_gpu_bsdf_grad_desc *desc, const nori_gpu_surface *surf,
                       const float *wi, const float *wo, const float *grad_out, float *grad_materials,
                       float *terms, nori_gpu_stats *stats);

/* The renderer's own random numbers, the companion of nori_gpu_camera_rays:
 * draws [first, first + count) of Sampler::next1D on the stream of sample
 * (pass pass_begin + k, pixel pix = y W + x), wave_seed(seed, (pass_begin + k)
 * W H + pix), written at out[count (k H W + pix) + j], j < count, for
 * k < pass_count and the pixels of the selected blocks (other entries are left
 * untouched).  out: pass_count x H x W x count floats (4-byte aligned on the
 * device).  A sample consumes its stream in this order: draws 0, 1 the pixel
 * jitter (x, y); 2, 3 the aperture sample -- drawn for every camera, used or
 * not; from draw 4 on the integrator's, in the order of its Li.  next2D is two
 * consecutive draws, x first.  direct_ems / direct_mis: one next2D per emitter
 * in index order, then (direct_mats, direct_mis) one next2D for the BSDF
 * sample.  Li of those integrators for a camera ray (o, d), every operation a
 * single float operation in the order written (a miss: 0):
 *   L = Emitter::eval at the hit seen from o        (nori_gpu_emitter_eval)
 *   per emitter i (direct_ems, direct_mis), with s = its next2D:
 *     (wi, maxt, Li, pdf_em) = nori_gpu_emitter_sample(p, s); skip if the
 *     shadow ray hits; (f, pdf_mat, cos) = nori_gpu_bsdf_eval(-d, wi);
 *     direct_ems: L = L + (f * cos) * Li
 *     direct_mis: w = pdf_mat + pdf_em > 0 ? pdf_em / (pdf_mat + pdf_em) : pdf_em;
 *                 L = L + ((f * w) * Li) * cos
 *   then (direct_mats, direct_mis), with s = the last next2D:
 *     (dir, pdf_mat, weight) = nori_gpu_bsdf_sample(-d, s); a zero weight ends
 *     it; the ray (p, NORI_EPSILON, dir, +inf) must hit a shape with an
 *     emitter, else it ends; (Le, pdf_em) = nori_gpu_emitter_eval there seen from p;
 *     direct_mats: L = L + weight * Le
 *     direct_mis:  w = pdf_mat + pdf_em > 0 ? pdf_mat / (pdf_mat + pdf_em) : 0;
 *                  L = L + (weight * w) * Le
 * (tests/shading_compose.py is this text in numpy; the per-pixel statistics of
 * a one-pass nori_gpu_render hold 0 + L of each sample.)
 * From `desc`: pass_begin, pass_count (0 = the scene's sampleCount),
 * seed, num_blocks / block_ids and output_on_device; the other fields are
 * ignored, variance_out must be NULL.  NORI_ERR_INVALID: a null argument,
 * count == 0, first + count overflowing 32 bits, variance_out set, a device
 * pointer that is misaligned or not device memory.  Blocking, on the context's
 * stream. */
int nori_gpu_sample_uniforms(nori_gpu_ctx *ctx, const nori_gpu_render_desc *desc, uint32_t first,
                             uint32_t count, float *out);

/* ---- radiance queries: Integrator::Li along the caller's rays ----
 * (the reference calls Li(scene, sampler, ray) one ray at a time,
 * include/nori/integrator.h:55; the batch form, its stream convention and its
 * chromatic rule are deviation D18)
 * The built-in integrators without the scene's camera, pixel grid and film:
 *   nori_gpu_camera_rays or your own rays -> nori_gpu_li -> nori_gpu_film_splat */
typedef struct nori_gpu_li_desc {
    uint32_t n;            /* rays */
    int32_t  on_device;    /* rays, stream_ids and out are device memory on the context's device */
    uint64_t seed;         /* as nori_gpu_render_desc.seed */
    uint64_t stream_base;  /* stream_ids == NULL: ray i draws from wave_seed(seed, stream_base + i) */
    uint32_t first_draw;   /* draws of that stream skipped before the integrator's first (<= 65535) */
    uint32_t reserved;     /* must be 0 */
} nori_gpu_li_desc;        /* 32 bytes */
/* Arrays.  rays: n x 8 floats (o.xyz, mint, d.xyz, maxt), 16-byte aligned on
 * the device, as for nori_gpu_query.  stream_ids: NULL, or n x uint64 (8-byte
 * aligned on the device): ray i then draws from wave_seed(seed, stream_ids[i]),
 * so that rays the caller has compacted or permuted keep their streams.  out:
 * n x 3 floats, packed (4-byte aligned on the device) -- the `val` layout of
 * nori_gpu_film_splat, which it feeds without a copy.
 * What is computed.  out[i] = Integrator::Li(scene, sampler, Ray3f(o, d, mint,
 * maxt)) of the context's integrator -- any of path_mis, path_mats, volumetric,
 * normals, av, direct, direct_ems, direct_mats, direct_mis, photonmapper -- with
 * the sampler being the pcg32 stream above after first_draw calls of next1D.
 * The first segment uses the ray's own mint and maxt, every later segment
 * (NORI_EPSILON, +inf) as in the renderer; d is used as given, not normalised.
 * The value is the one the render kernels compute for a camera sample that
 * starts with this ray: the same routines, the same order of the draws
 * (nori_gpu_sample_uniforms lists it) and the same order of the additions,
 * which start from +0 and add, per path vertex, the emission first and then
 * the next-event term if its shadow ray is unoccluded.  The result of a ray
 * depends on its eight floats, its stream and first_draw only -- not on n, on
 * its place in the batch, or on NORI_LI_RANGE / NORI_LI_REFILL below.
 * The renderer's samples.  For a camera without chromatic aberration, take the
 * rays of nori_gpu_camera_rays(pass_begin = p, pass_count = k, seed = s) as
 * k H W rows and call nori_gpu_li with seed = s, stream_base = p W H and
 * first_draw = 4 (draws 0..3 are the pixel jitter and the aperture sample):
 * out holds exactly the radiance of the samples nori_gpu_render takes for
 * those passes -- the values its variance_out statistics add to +0.  A
 * chromatic sample cannot be reproduced this way: the renderer calls Li three
 * times on one stream, once per channel's ray, and keeps one channel of each.
 * Chromatic aberration is a property of the camera, and Li knows no camera:
 * nori_gpu_li returns all three channels of every ray, also on a context whose
 * camera has chromaticAberation set.
 * Invalid values.  A value that is negative or not finite is written as
 * computed (nori_gpu_film_splat drops and counts it, as block.cpp:94-98 does)
 * and its row is counted in stats->invalid_samples.  A ray is not traced, and
 * its row is three zeros (a valid value), when a component of o or d, or mint,
 * is not finite, when maxt is NaN, or when d is zero: nori_gpu_camera_rays
 * leaves the entries of unselected blocks untouched, so all-zero rays are an
 * expected input.  (A ray with maxt < mint is traced and hits nothing.)
 * NORI_ERR_INVALID, nothing launched, the context stays usable: a null ctx,
 * desc, rays or out; reserved != 0; first_draw > 65535; on_device with a
 * pointer that is misaligned or that the HIP runtime does not know as device
 * memory.  n == 0 is a no-op.
 * Host arrays are staged through context-owned buffers in chunks of at most
 * NORI_QUERY_CHUNK rays; device arrays are used in place, nothing is allocated
 * per call, and the caller has made them ready before the call.  Blocking; runs
 * on the context's stream in launches of at most 16M rays, between which
 * nori_gpu_cancel is honoured (NORI_ERR_CANCELLED; a host `out` is left
 * unchanged then, a device `out` holds the launches that ran) and over which
 * nori_gpu_progress rises.  After nori_gpu_update_vertices /
 * nori_gpu_rebuild_bvh it answers for the geometry as it is now.
 * stats (may be NULL): samples = n, invalid_samples, rays_closest, rays_shadow,
 * ms_total (wall time), ms_shade = HIP-event time of the kernel.
 * Environment, read at every call: NORI_LI_RANGE (64 .. 4096, default 256) --
 * the consecutive rays one wave owns; a lane whose path has ended starts the
 * next ray of its wave's range; NORI_LI_REFILL=0 -- every lane takes exactly
 * one ray instead (the A/B of that refill). */
int nori_gpu_li(nori_gpu_ctx *ctx, const nori_gpu_li_desc *desc, const float *rays,
                const uint64_t *stream_ids, float *out, nori_gpu_stats *stats);

/* ---- film splat: caller-supplied samples filtered into the film ----
 * (no reference counterpart as an API: it is ImageBlock::put(pos, value)
 * followed by put(block), the step the built-in integrators end with;
 * deviation D17)
 * The statement, on the host.  pos: n x 2 floats, the sample position in pixel
 * units (the reference's pixelSample; for the renderer's own samples
 * (float)x + u0, (float)y + u1 with u0, u1 draws 0 and 1 of
 * nori_gpu_sample_uniforms); val: n x 3 floats; rgbw: (H+2b) x (W+2b) x 4,
 * ADDED into; stats: NULL or H x W x 8, added into, laid out as
 * nori_gpu_render_desc.variance_out.  For each sample i, in index order:
 *  1. Owner pixel (x, y).  ordered == 0: (floor(pos.x), floor(pos.y)).
 *     ordered != 0: n is a multiple of H W and the owner is pixel i mod (H W),
 *     the layout of nori_gpu_camera_rays (pass k at k H W + y W + x); the
 *     position must lie in the closed square [x, x+1] x [y, y+1] (closed:
 *     (float)x + u can round up to x + 1).
 *  2. The sample is dropped and counted in counts[1] if the position is not
 *     finite, the owner is outside the frame, (ordered) the position is
 *     outside the owner's square, or val fails Color3f::isValid (a channel
 *     negative or not finite).
 *  3. Otherwise it is counted in counts[0] and put into the owner's 32x32
 *     frame block (block.cpp:93-122), origin (ox, oy), size bw x bh (smaller
 *     at the frame's edge): px = pos.x - 0.5f - (float)(ox - b), py likewise;
 *     the window runs from ceil(px - radius) to floor(px + radius), clipped to
 *     the block's own tile [0, bw + 2b - 1] (and [0, bh + 2b - 1]); the
 *     weights are table[min((int)(fabsf((float)c - px) * lookup),
 *     NORI_FILTER_RESOLUTION)], lookup = NORI_FILTER_RESOLUTION / radius; cell
 *     (ox + cx, oy + cy) of rgbw receives (val.c * wx) * wy for c = r, g, b and
 *     (1.0f * wx) * wy -- each a single float operation in the order written.
 *  4. With stats, the owner's floats 0..6 receive L.r, L.g, L.b, L.r L.r,
 *     L.g L.g, L.b L.b and 1.
 * The device calls below produce the same terms bit for bit and may differ
 * only in the order of the additions.  NORI_ERR_INVALID: a null argument
 * (stats may be NULL), ordered with n not a multiple of H W. */
int nori_film_splat(const nori_scene_desc *scene, uint64_t n, int ordered, const float *pos,
                    const float *val, float *rgbw, float *stats, uint64_t counts[2]);

typedef struct nori_gpu_splat_desc {
    uint64_t n;                   /* samples                                   */
    int32_t on_device;            /* pos, val, rgbw and variance_out are device
                                     memory on the context's device            */
    uint32_t reserved;            /* must be 0                                 */
    float *variance_out;          /* optional H x W x 8, added into            */
} nori_gpu_splat_desc;

/* nori_film_splat on the context's device, for a context of any integrator and
 * traversal mode.  Device arrays are used in place (pos and val 4-byte, rgbw
 * and variance_out 16-byte aligned, all checked to be device memory); host
 * arrays are staged through context-owned buffers in chunks of at most
 * NORI_QUERY_CHUNK samples (the passes layout: whole passes, at least one), and
 * a host film is accumulated on the device and added into the caller's array
 * once, as nori_gpu_render does.  stats (may be NULL): samples = splatted,
 * invalid_samples = dropped, ms_total, ms_splat = HIP-event time of the
 * kernels.  Blocking, on the context's stream.  A refusal launches nothing and
 * leaves the context usable.
 * nori_gpu_film_splat: samples anywhere on the image, nori_film_splat with
 * ordered = 0.  n == 0 is a no-op.  NORI_ERR_INVALID: a null argument, reserved
 * != 0, a device pointer that is misaligned or not device memory. */
int nori_gpu_film_splat(nori_gpu_ctx *ctx, const nori_gpu_splat_desc *desc, const float *pos,
                        const float *val, float *rgbw, nori_gpu_stats *stats);
/* nori_gpu_film_splat_passes: samples in the layout of nori_gpu_camera_rays,
 * nori_film_splat with ordered = 1 -- pos: pass_count x H x W x 2, val:
 * pass_count x H x W x 3.  From `desc`: pass_count (0 = the scene's
 * sampleCount), num_blocks / block_ids (only the selected blocks' pixels are
 * read and splatted, the rest of a device array is never touched),
 * output_on_device (which covers pos, val, rgbw and variance_out) and
 * variance_out; pass_begin, seed, path_pool and timing are ignored.
 * NORI_ERR_INVALID: a null argument, a block id out of range, no passes (both
 * pass_count and the scene's sampleCount 0), a device pointer that is
 * misaligned or not device memory. */
int nori_gpu_film_splat_passes(nori_gpu_ctx *ctx, const nori_gpu_render_desc *desc, const float *pos,
                               const float *val, float *rgbw, nori_gpu_stats *stats);

/* ---- film gather: the film splat's adjoint ----
 * (no reference counterpart; deviation D19)
 * nori_film_splat is linear in val; its adjoint is a gather: every sample reads
 * the film cells of its own window with the weights it was splatted with.
 * The statement, on the host.  pos: n x 2 floats; val: n x 3 floats or NULL;
 * grad_rgbw: (H+2b) x (W+2b) x 4, read only -- channel 3 is never read, the
 * weight channel of the splat does not depend on val; grad_val: n x 3 floats,
 * WRITTEN, not added into.  For each sample i:
 *  1. Steps 1 and 2 of nori_film_splat decide the owner and whether the sample
 *     is kept: the position, the owner and, with val != NULL, Color3f::isValid
 *     of val[i].  A dropped sample gets the row (0, 0, 0) and is counted in
 *     counts[1] (it added nothing to the film, so its derivative is zero); a
 *     kept one is counted in counts[0].
 *  2. A kept sample uses the window and the weights of step 3 there (px, py,
 *     the window clipped to the owner block's tile, wx, wy from the table).
 *     For c = r, g, b: acc = 0.0f; for cy ascending, then cx ascending:
 *     acc = acc + (G[c] * wx) * wy, G = cell (ox + cx, oy + cy) of grad_rgbw,
 *     each a single float operation in the order written;
 *     grad_val[3 i + c] = acc.  An empty window gives zeros.
 * pos gets no derivative: the tabulated filter is piecewise constant in the
 * position.  The device calls below produce the same float32 terms
 * (G[c] * wx) * wy bit for bit and may differ only in the order of a sample's
 * additions.  NORI_ERR_INVALID: a null argument (val may be NULL), an empty
 * frame, ordered with n not a multiple of H W. */
int nori_film_gather(const nori_scene_desc *scene, uint64_t n, int ordered, const float *pos,
                     const float *val, const float *grad_rgbw, float *grad_val, uint64_t counts[2]);

typedef struct nori_gpu_gather_desc {
    uint64_t n;                   /* samples                                   */
    int32_t on_device;            /* pos, val, grad_rgbw and grad_val are device
                                     memory on the context's device            */
    uint32_t reserved;            /* must be 0                                 */
} nori_gpu_gather_desc;

/* nori_film_gather on the context's device, for a context of any integrator and
 * traversal mode.  Device arrays are used in place (pos, val and grad_val
 * 4-byte, grad_rgbw 16-byte aligned, all checked to be device memory).  Of
 * host arrays grad_rgbw is copied once into a context-owned buffer, pos and val
 * are staged in chunks of at most NORI_QUERY_CHUNK samples (the passes layout:
 * whole passes, at least one) and each chunk's rows are copied back.  val may
 * be NULL.  stats (may be NULL): samples = kept, invalid_samples = zero rows,
 * ms_total, ms_splat = HIP-event time of the kernels.  Blocking, on the
 * context's stream.  A refusal launches nothing and leaves the context usable.
 * nori_gpu_film_gather: samples anywhere on the image (ordered = 0).  n == 0 is
 * a no-op.  NORI_ERR_INVALID: a null argument, reserved != 0, a device pointer
 * that is misaligned or not device memory. */
int nori_gpu_film_gather(nori_gpu_ctx *ctx, const nori_gpu_gather_desc *desc, const float *pos,
                         const float *val, const float *grad_rgbw, float *grad_val,
                         nori_gpu_stats *stats);
/* nori_gpu_film_gather_passes: the layout of nori_gpu_camera_rays (ordered = 1)
 * -- pos: pass_count x H x W x 2, val (or NULL) and grad_val: pass_count x H x
 * W x 3.  From `desc`: pass_count (0 = the scene's sampleCount), num_blocks /
 * block_ids (only the selected blocks' pixels are read and written, every other
 * entry of grad_val is left untouched) and output_on_device (which covers all
 * four arrays); the other fields are ignored.  NORI_ERR_INVALID: as
 * nori_gpu_film_splat_passes.  Environment, read at every call:
 * NORI_GATHER_PASSES -- the passes one work-group walks (default: at most 4). */
int nori_gpu_film_gather_passes(nori_gpu_ctx *ctx, const nori_gpu_render_desc *desc, const float *pos,
                                const float *val, const float *grad_rgbw, float *grad_val,
                                nori_gpu_stats *stats);

/* ---- dynamic geometry: new vertex positions, the BVH refitted on the device ----
 * (no reference counterpart: the reference builds its BVH once, in
 * Scene::activate; deviation D14) */
typedef struct nori_gpu_update_desc {
    const float *positions;  /* num_vertices x 3 floats, required                              */
    const float *normals;    /* num_vertices x 3 floats, or NULL: the vertex normals stay      */
    uint32_t num_vertices;   /* must equal the scene's num_vertices                            */
    int32_t  on_device;      /* both pointers are device memory on the context's device        */
    uint32_t reserved[4];    /* must be 0 */
} nori_gpu_update_desc;
typedef struct nori_gpu_update_stats {
    float ms;                /* wall time of the call (host timer)                              */
    float ms_device;         /* HIP-event time of the vertex, record and refit launches         */
    float root_min[3], root_max[3];  /* the scene box after the refit                          */
    uint32_t nodes;          /* 4-wide nodes refitted                                           */
    uint32_t levels;         /* refit launches (the levels of the schedule)                     */
    uint32_t launches;       /* kernel launches of the call in all                              */
    uint32_t reserved;
} nori_gpu_update_stats;

/* The refit's one statement, on the host (no device needed); the kernels of
 * nori_gpu_update_vertices are tested against it byte for byte.  Builds the
 * scene's device BVH exactly as nori_gpu_create does (node and primitive
 * counts: nori_scene_bvh_info's device_nodes and num_prims) and refits it to
 * `positions` (num_vertices x 3 floats; NULL: the tree as built, nothing
 * refitted):
 *   - topology, child refs, leaf ranges and leaf order do not change;
 *   - a triangle's record becomes (p0 | id), (p1 - p0 | w), (p2 - p0 | w) with
 *     p0, p1, p2 its vertices' new positions and every w word as it was; a
 *     sphere's record stays (spheres do not move: centre and radius belong to
 *     the shape);
 *   - the box of a leaf child is the component-wise min / max of the vertex
 *     POSITIONS of its triangles (not of v0 + e1, which can differ by an ulp)
 *     and of centre -/+ radius of its spheres; the box of an inner child is
 *     the min / max over the used slots of that child node;
 *   - an unused child slot is the one whose box is NaN (its ref, the leaf bit
 *     alone, is also the valid ref of a one-primitive leaf at record 0); it is
 *     never written and stays NaN;
 *   - min and max order the zeros, -0 < +0, so a box depends on the set of its
 *     points only; they do not round: any correct implementation gives the
 *     same bytes.
 * nodes: 32 floats per node, prims: 12 floats per primitive record (the
 * layouts of nori_gpu_bvh_read), root_box: min.xyz, max.xyz over the root
 * node's used slots -- the min / max over all primitives; each may be NULL.
 * The statement has no memory: the result depends on the scene and on
 * `positions` only.  NORI_ERR_INVALID: a null scene, a non-finite position. */
int nori_scene_bvh_refit(const nori_scene_desc *scene, const float *positions, float *nodes, float *prims,
                         float root_box[6]);

/* Moves the context's mesh vertices to desc->positions (and, if given, sets
 * their normals) and refits the BVH as nori_scene_bvh_refit states, all on the
 * device: pos.xyz / nrm.xyz are rewritten (their w lanes, the texture
 * coordinates, stay), the triangle records rebuilt, the boxes refitted level
 * by level (one launch per level of a schedule made at nori_gpu_create), and
 * what the lights derive from the geometry recomputed -- for every mesh that
 * carries an emitter the area CDF and its normalisation, in
 * nori_gpu_create's own fp32 order (on the host, from a read-back of those
 * meshes' vertices: a refitted context samples its lights bit-identically to
 * a fresh one on the same positions).  The CDF of a mesh without an emitter
 * is read by no kernel and goes stale.  The scene box becomes the refitted
 * root box.  Every sphere's `solitary` shortcut (an exact shortcut of the
 * tail finisher whose precondition, no other primitive near the ball, was
 * checked against the geometry as loaded) is switched off for good.  Every
 * later render, feature pass, trace and query of the context sees the new
 * geometry; hit distances and barycentrics are those of a context created
 * fresh on the same positions, bit for bit (they depend on the triangle
 * record alone), at the traversal cost of a tree whose topology was chosen
 * for the old positions.
 * Host arrays are staged through context-owned device buffers; with on_device
 * the pointers are used in place (4-byte aligned; the caller has made them
 * ready before the call) and nothing is copied.  Blocking; runs on the
 * context's stream: concurrent use with a render or query of the same context
 * is not supported.  The host nori_scene is not touched: nori_scene_surface,
 * nori_scene_bvh_refit(.., NULL, ..) and the scene's arrays keep describing
 * the geometry as loaded.
 * Refused with nothing changed (the context renders exactly as before):
 * NORI_ERR_UNSUPPORTED -- a scan-mode context (its scan list, axis-plane
 *   pairs and specialised kernels are functions of the geometry: create the
 *   context with NORI_TRAVERSAL=bvh), a photonmapper context (its photon map
 *   was traced at creation);
 * NORI_ERR_INVALID -- a null ctx, desc or positions, num_vertices other than
 *   the scene's, reserved != 0, an on_device pointer that is not 4-byte
 *   aligned or that the HIP runtime does not know as device memory, any non-finite position or normal (counted on the device in a
 *   pass of its own before anything is modified, device buffers included).
 * stats may be NULL. */
int nori_gpu_update_vertices(nori_gpu_ctx *ctx, const nori_gpu_update_desc *desc, nori_gpu_update_stats *stats);
/* ---- dynamic geometry: the BVH rebuilt for the positions as they are now ----
 * (deviation D15).  A refit keeps the topology the SAH builder chose
 * for the positions as loaded; after a large displacement that tree traces
 * slowly.  The rebuild is a linear BVH -- Morton keys, a sort, a radix tree
 * emitted 4-wide -- stated here once and reproduced by the kernels of
 * nori_gpu_rebuild_bvh byte for byte.  The tree is a function of the scene,
 * the positions and leaf_max only; every step is integer arithmetic or fp32
 * with a stated operation order (contraction is off in this build), so any
 * correct implementation gives the same bytes.
 *
 * Primitive boxes.  Primitives are numbered by their global id, in shape
 *   order; a sphere is one primitive.  A triangle's box is the box_min /
 *   box_max (min / max with ordered zeros, -0 < +0, as in the refit) over its
 *   three vertex positions; a sphere's is centre -/+ radius in fp32.  The scene
 *   box Lo, Hi is the box_min / box_max over all primitive boxes.
 * Keys.  Per axis, in fp32: c = 0.5f * lo + 0.5f * hi of the primitive's box,
 *   ext = Hi - Lo, scale = ext > 0 ? 1024.0f / ext : 0.0f (one correctly
 *   rounded division), x = (c - Lo) * scale,
 *   q = !(x >= 0) ? 0 : x >= 1023 ? 1023 : (uint32_t)x   (a NaN from inf * 0
 *   gives 0).  The 30-bit Morton code has bit 3k+2 = bit k of qx, bit 3k+1 =
 *   bit k of qy, bit 3k = bit k of qz.  The sort key is the 64-bit
 *   code << 32 | id: keys are unique, so every correct sort gives the same
 *   order.  Leaf order is ascending key.
 * Records.  The ones nori_gpu_create writes for the same positions, in the new
 *   leaf order: triangle (p0 | id), (p1 - p0 | 0), (p2 - p0 | 0); sphere
 *   (centre | id), (r, 0, 0, 1), 0.
 * Topology.  Let K[i] = code_i << 32 | i with i the position in leaf order.  A
 *   range [a, b] of more than leaf_max records is split after g, the largest
 *   index in [a, b) whose K shares more leading bits with K[a] than K[b] does
 *   (Karras 2012); equal codes therefore split on the bits of the position, so
 *   a cluster of ties gets a balanced subtree.  A range of at most leaf_max
 *   records is a leaf, its ref leaf bit | (count - 1) << 25 | first.  The
 *   4-wide node of a range R takes R's two halves and replaces every half that
 *   is not a leaf by its own two halves, in place and in order: 2 to 4 used
 *   slots, filled from slot 0; unused slots get the ref `leaf bit` and a NaN
 *   box.  The root is node 0; when n <= leaf_max it has one leaf slot.  Nodes
 *   are numbered breadth-first: the nodes of depth d + 1 follow those of depth
 *   d, ordered by (parent number, slot).  `depth` is the number of levels.
 * Boxes.  Exactly what nori_scene_bvh_refit states on this topology: leaf
 *   slots from the vertex positions with ordered zeros, inner slots from the
 *   child's used slots; root_box as there.
 *
 * positions: num_vertices x 3 floats, NULL = the scene's own.  leaf_max:
 * 1 .. 64, 0 = the default, 4.  refit_positions (optional): the finished tree
 * is then refitted to them exactly as nori_scene_bvh_refit states (what a
 * nori_gpu_update_vertices after a nori_gpu_rebuild_bvh gives).  info, nodes
 * (32 floats per node), prims (12 floats per record) and root_box may each be
 * NULL: call with info alone for the sizes.  NORI_ERR_INVALID: a null scene, a
 * non-finite position, leaf_max > 64. */
typedef struct nori_bvh_rebuild_info {
    uint32_t device_nodes, depth, num_prims, leaf_max;  /* leaf_max: the value used */
    uint32_t reserved[4];
} nori_bvh_rebuild_info;
int nori_scene_bvh_rebuild(const nori_scene_desc *scene, const float *positions, uint32_t leaf_max,
                           const float *refit_positions, nori_bvh_rebuild_info *info, float *nodes, float *prims,
                           float root_box[6]);

typedef struct nori_gpu_rebuild_desc {
    uint32_t leaf_max;       /* 1 .. 64; 0 = the default, 4 */
    uint32_t reserved[7];    /* must be 0 */
} nori_gpu_rebuild_desc;
typedef struct nori_gpu_rebuild_stats {
    float ms;                /* wall time of the call (host timer)                    */
    float ms_device;         /* HIP-event time from the first launch to the last      */
    uint32_t nodes, depth;   /* the new tree: 4-wide nodes, levels                    */
    uint32_t stack;          /* the traversal stack now in use (8, 16 or 32)          */
    uint32_t levels;         /* levels of the new refit schedule                      */
    uint32_t launches;       /* kernel launches of this library (the sort's and the scan's own not counted) */
    uint32_t reserved;
} nori_gpu_rebuild_stats;
/* Rebuilds the context's BVH on the vertex positions the context holds now
 * (as created, or as set by the last nori_gpu_update_vertices), all on the
 * device: the result is byte for byte nori_scene_bvh_rebuild's tree for those
 * positions (nori_gpu_bvh_read shows it).  The scene box is reduced with
 * integer atomics on an order-preserving key, the keys are sorted with
 * rocprim's radix sort, the tree is emitted one breadth-first level per
 * launch set (the host reads one pair of counts back per level and checks it
 * against its bound before it sizes the next launches) and the boxes are
 * fitted by the refit's own kernel.  Everything is built in scratch buffers
 * of the context; on success the nodes, the records, the refit schedule, the
 * depth, node count, traversal stack (nori_gpu_create's rule for the new
 * depth; a stack forced by NORI_BVH_STACK at creation stays forced) and the
 * scene box are replaced together, and later nori_gpu_update_vertices calls
 * refit the rebuilt tree.  The light CDFs, the spheres' `solitary` flags, the
 * vertex buffers and everything else stay.  Hit distances and barycentrics
 * are those of any other tree over the same records, bit for bit.
 * Blocking; runs on the context's stream: concurrent use with a render or
 * query of the same context is not supported.
 * Refused with nothing changed (the context traces and renders exactly as
 * before):
 * NORI_ERR_UNSUPPORTED -- a scan-mode context (create it with
 *   NORI_TRAVERSAL=bvh), a photonmapper context (the same surface as
 *   nori_gpu_update_vertices), a tree too deep for the traversal stack
 *   (binary depth is at most 30 + ceil(log2 n), the 4-wide depth about half
 *   of it: ordinary scenes are far inside the limit);
 * NORI_ERR_INVALID -- a null ctx or desc, leaf_max > 64, reserved != 0.
 * stats may be NULL. */
int nori_gpu_rebuild_bvh(nori_gpu_ctx *ctx, const nori_gpu_rebuild_desc *desc, nori_gpu_rebuild_stats *stats);

/* The context's own shade kernel (nori_scene_shade_rtc): *active = 1 if
 * renders launch it in place of the ahead-of-time kernel (0 for BVH and
 * full-plugin scenes, under NORI_RTC=0 or NORI_RTC_SHADE=0, and after any
 * failure to compile, load or match its argument layout), *cached = 1 if its
 * code object came from the process or disk cache, *ms = the compile or cache
 * read time paid at nori_gpu_create, *code_bytes = the code object's size.
 * Any output may be null.  nori_gpu_stats keeps its layout: scan_rtc and
 * ms_scan_rtc there speak of the scan program alone. */
int nori_gpu_shade_rtc_info(nori_gpu_ctx *ctx, int *active, int *cached, double *ms, size_t *code_bytes);
/* Introspection for tests, like nori_scene_scan_list: the context's BVH nodes
 * (32 floats per node) and primitive records (12 floats per record, leaf
 * order; a scan-mode context holds its scan list there) as they are on the
 * device.  counts (may be NULL) receives the node and record counts; nodes and
 * prims may each be NULL (call with both NULL for the counts).  Blocking. */
int nori_gpu_bvh_read(nori_gpu_ctx *ctx, float *nodes, float *prims, uint32_t counts[2]);
int nori_gpu_cancel(nori_gpu_ctx *ctx);
float nori_gpu_progress(const nori_gpu_ctx *ctx);
void nori_gpu_destroy(nori_gpu_ctx *ctx);

/* ---- multi-GPU: one process per GPU, film sum over RCCL -------------------
 * Samples are independent, so a frame shards without any data-path
 * collective; the only exchange is the final film sum.  librccl is opened at
 * run time from the directory of the process's HIP runtime (fallback:
 * librccl.so.1); without it these calls fail with NORI_ERR_UNSUPPORTED and
 * everything else works. */
typedef struct nori_gpu_comm nori_gpu_comm;
#define NORI_COMM_ID_BYTES 128
/* Rank 0 makes the communicator id (ncclGetUniqueId); the caller hands the
 * bytes to every rank over any channel (torch.distributed store, MPI, file). */
int nori_gpu_comm_id(unsigned char id[NORI_COMM_ID_BYTES]);
/* Collective over the nranks processes (ncclCommInitRank); device = this
 * process's GPU (the device of the contexts used with the communicator). */
int nori_gpu_comm_create(const unsigned char id[NORI_COMM_ID_BYTES], int nranks, int rank, int device,
                         nori_gpu_comm **out);
int nori_gpu_comm_rank(const nori_gpu_comm *comm, int *nranks, int *rank);
void nori_gpu_comm_destroy(nori_gpu_comm *comm);
/* Path of the librccl opened (loading it if needed), NULL if none loads. */
const char *nori_gpu_comm_library(void);

#define NORI_SHARD_PASSES 0  /* rank r: passes [P*r/N, P*(r+1)/N) of every block (default) */
#define NORI_SHARD_BLOCKS 1  /* rank r: blocks r, r+N, r+2N, ... of the BlockGenerator's spiral
                                order (block.cpp:140-188), every pass */
/* The share of a whole-frame render `desc` that rank `rank` of `nranks`
 * renders: writes this rank's pass range and block ids into *out and
 * block_buf (capacity = the frame's block count).  desc->num_blocks != 0
 * restricts the frame to those blocks first (ids checked against the frame,
 * duplicates dropped); desc->pass_count == 0 means the scene's sampleCount.
 * out->pass_count == 0: the rank has no share (more ranks than passes /
 * blocks).  Pure host function. */
int nori_gpu_shard_desc(const nori_scene_desc *scene, const nori_gpu_render_desc *desc, int mode, int nranks,
                        int rank, nori_gpu_render_desc *out, uint32_t *block_buf);
/* Render this rank's share of `desc` into film_dev (device memory on the
 * context's device, (H+2b)x(W+2b)x4 floats; ZEROED first) and sum the films
 * of all ranks on the context's stream: into root's film_dev (ncclReduce), or
 * into every rank's when root < 0 (ncclAllReduce).  Returns after the sum has
 * completed on this rank.  stats: this rank's share.  desc->variance_out must
 * be NULL (per-pixel statistics are not summed across ranks).
 * Failure handling: every rank joins a status exchange before the film sum.
 * If any rank's share was cancelled (nori_gpu_cancel) every rank returns
 * NORI_ERR_CANCELLED; if any failed (bad arguments, allocation, a HIP error
 * that leaves the device usable, any exception of the render), the failing
 * rank returns its error and the others NORI_ERR_INVALID ("the frame is
 * incomplete"); no film sum runs and the communicator stays usable.  A rank
 * whose device faulted (a sticky HIP error) cannot join: it aborts the
 * communicator (ncclCommAbort) and returns NORI_ERR_HIP.  Its peers, and any
 * rank whose peers do not reach a collective, give up after the watchdog
 * bound nori_gpu_comm_timeout(own status, own render seconds, own samples,
 * largest share's samples) -- max(30 s, 20 x the own render time scaled to
 * the largest share) after a rendered share, 600 s for a rank whose share
 * failed, was cancelled or is empty, NORI_COMM_TIMEOUT_S seconds if set --
 * abort and return NORI_ERR_HIP; an aborted communicator fails every later
 * call. */
int nori_gpu_render_sharded(nori_gpu_ctx *ctx, nori_gpu_comm *comm, const nori_gpu_render_desc *desc, int mode,
                            int root, float *film_dev, nori_gpu_stats *stats);
/* The status word a rank contributes to the exchange (reduced by max):
 * severity << 16 | rank, severity 0 for NORI_OK, 1 for NORI_ERR_CANCELLED,
 * 2 for any other status.  Pure function. */
int nori_gpu_comm_status_word(int status, int rank);
/* The watchdog bound of a sharded render's collectives, in seconds (see
 * nori_gpu_render_sharded); status = the rank's own share's outcome.  Pure
 * function (reads NORI_COMM_TIMEOUT_S). */
double nori_gpu_comm_timeout(int status, double own_seconds, double own_samples, double max_samples);

#ifdef __cplusplus
}
#endif
#endif /* NORI_GPU_H */
