/*
 * soc_rt.h — C ABI of the MI355X-native screen-space deferred-shading and post-processing
 * passes of lukasino1214/soc_real_time_renderer.
 *
 * Every entry point below replaces ONE render-graph task of the reference (a Daxa task struct whose
 * callback() records a fullscreen draw / compute dispatch). The reference file:line of the task that
 * each function replaces is cited next to it. Shader-level semantics (sampling, formats, quirks
 * Q1..Q12 of SURVEY.md §8a) are documented in DESIGN.md.
 *
 * Conventions:
 *   - The caller owns all device memory. No function allocates on the hot path, and none keeps a
 *     pointer after it returns.
 *   - Calls are stream-ordered and asynchronous on the given HIP stream; the caller synchronises.
 *   - Return value: 0 on success, < 0 on error (SOC_E_*); soc_last_error_string() gives the
 *     message of the calling thread's last error. No C++ exception crosses this ABI.
 *   - Images are pitch-linear, row-major, y = 0 is the TOP row (the reference's uv.y = 0).
 *   - `const soc_globals* g` is a HOST pointer to the per-frame globals (mirror of ShaderGlobals,
 *     src/graphics/shared.inl:47-131). Only the fields a pass reads are consumed; they are packed
 *     into the kernel arguments at call time (the reference memcpy's the whole block into a UBO
 *     ring slot, src/graphics/renderer.cpp:648-657).
 */
#ifndef SOC_RT_H
#define SOC_RT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOC_RT_ABI_VERSION 1

/* Error codes. */
#define SOC_OK 0
#define SOC_E_INVALID_ARG (-1)   /* null pointer, bad format, bad extent            */
#define SOC_E_SHAPE (-2)         /* image extents inconsistent with the pass        */
#define SOC_E_HIP (-3)           /* a HIP runtime call failed (launch, memcpy, ...) */
#define SOC_E_UNSUPPORTED (-4)   /* format / configuration not implemented          */

struct ihipStream_t;
typedef struct ihipStream_t* soc_stream; /* == hipStream_t; NULL = the null stream */

/* Image formats: the reference's Vulkan formats (src/graphics/renderer.cpp:348-470). */
typedef enum soc_format {
    SOC_FMT_RGBA16F = 1,     /* R16G16B16A16_SFLOAT, 8 B/px (albedo, emissive, normal, color, velocity, bloom mips) */
    SOC_FMT_D32F = 2,        /* D32_SFLOAT, 4 B/px (depth, sun shadow map)                                      */
    SOC_FMT_R8_UNORM = 3,    /* R8_UNORM, 1 B/px (ssao, ssao blur)                                              */
    SOC_FMT_RGBA8_UNORM = 4, /* R8G8B8A8_UNORM, 4 B/px (clouds, noise texture, headless swapchain)              */
    SOC_FMT_RGBA8_SRGB = 5,  /* R8G8B8A8_SRGB, 4 B/px (optional headless swapchain with sRGB encode on store)   */
    SOC_FMT_RGBA32F = 6      /* R32G32B32A32_SFLOAT, 16 B/px (debug / exact tone-map output)                     */
} soc_format;

/* A borrowed view of a 2-D image in device memory (host memory for the CPU oracle): pitch-linear rows, so a view
 * into a wider allocation (padded rows, a column offset) is an image. With bpp = bytes_per_pixel(format):
 *  - `data` and `pitch_bytes` are multiples of bpp (every kernel loads and stores whole texels); an image that is
 *    not is refused with SOC_E_INVALID_ARG. Nothing more is required: launchers choose wider loads / stores from
 *    data % 16 and pitch_bytes % 16 themselves, with the same results.
 *  - A pass writes only the bytes [y * pitch_bytes, y * pitch_bytes + width * bpp) of each row y of an image it
 *    writes, and no byte of an image it only reads.
 *  - The library may read, but never uses, the bytes between the rows up to data + pitch_bytes * height (a wide
 *    load at a row's end, a buffer descriptor over the whole view): that range must be readable memory, whatever it
 *    holds (NaN, another image's texels) does not reach any result.
 * tests/test_gpu_views.py holds every pass to this on padded, offset and misaligned views. */
typedef struct soc_img {
    void* data;
    int32_t width;
    int32_t height;
    int32_t pitch_bytes; /* bytes between rows; >= width * bpp and a multiple of bpp */
    int32_t format;      /* soc_format */
} soc_img;

/* --- Globals: POD mirror of ShaderGlobals (src/graphics/shared.inl:5-131). ----------------------
 * Matrices are glm-layout column-major float[16] (m[col*4 + row]). Daxa sampler / image ids and the
 * AutoExposure buffer pointer are not part of this struct: samplers are fixed by the pass contract
 * (DESIGN.md "Sampling contract") and images/buffers are explicit arguments. */
typedef struct soc_point_light {   /* shared.inl:5-9 */
    float position[3];
    float color[3];
    float intensity;
} soc_point_light;

typedef struct soc_spot_light {    /* shared.inl:13-20 */
    float position[3];
    float direction[3];
    float color[3];
    float intensity;
    float cut_off;
    float outer_cut_off;
} soc_spot_light;

typedef struct soc_sun_info {      /* shared.inl:24-37 */
    float projection_matrix[16];
    float view_matrix[16];
    float projection_view_matrix[16];
    float terrain_y_clip_trick[4];
    float position[3];
    float direction[3];
    float exponential_factor;
    float darkening_factor;
    float bias;
    float intensity;
} soc_sun_info;

#define SOC_MAX_POINT_LIGHTS 128
#define SOC_MAX_SPOT_LIGHTS 128
#define SOC_AUTO_EXPOSURE_BIN_COUNT 256
#define SOC_SSAO_MAX_KERNEL 26

typedef struct soc_globals {       /* shared.inl:47-131 */
    float camera_projection_matrix[16];
    float camera_inverse_projection_matrix[16];
    float camera_view_matrix[16];
    float camera_inverse_view_matrix[16];
    float camera_projection_view_matrix[16];
    float camera_inverse_projection_view_matrix[16];

    float camera_previous_projection_matrix[16];
    float camera_previous_inverse_projection_matrix[16];
    float camera_previous_view_matrix[16];
    float camera_previous_inverse_view_matrix[16];
    float camera_previous_projection_view_matrix[16];
    float camera_previous_inverse_projection_view_matrix[16];

    float jitter[2];
    float previous_jitter[2];

    float camera_position[3];
    float camera_near_clip;
    float camera_far_clip;

    int32_t resolution[2];
    float elapsed_time;
    float delta_time;
    uint32_t frame_counter;

    soc_sun_info sun_info;

    uint32_t point_light_count;
    uint32_t spot_light_count;
    soc_point_light point_lights[SOC_MAX_POINT_LIGHTS];
    soc_spot_light spot_lights[SOC_MAX_SPOT_LIGHTS];

    float terrain_offset[3];
    float terrain_scale[2];
    float terrain_height_scale;
    float terrain_midpoint;
    float terrain_delta;
    float terrain_min_depth;
    float terrain_max_depth;
    int32_t terrain_min_tess_level;
    int32_t terrain_max_tess_level;
    float terrain_y_clip_trick[4];
    float terrain_previous_y_clip_trick[4];

    float filter_radius;           /* bloom (unused by the reference shaders) */

    float ssao_bias;
    float ssao_radius;
    int32_t ssao_kernel_size;

    float ambient[3];
    float ambient_occlussion_strength;
    float emissive_bloom_strength;

    float focal_length;            /* depth of field (disabled in the reference graph; soc_depth_of_field) */
    float plane_in_focus;
    float aperture;

    float adjustment_speed;
    float log_min_luminance;
    float log_max_luminance;
    float target_luminance;

    float saturation;
    float agxDs_linear_section;
    float peak;
    float compression;
} soc_globals;

/* AutoExposure buffer (shared.inl:39-45), device memory, caller-owned. */
typedef struct soc_auto_exposure {
    float exposure;
    uint32_t histogram_buckets[SOC_AUTO_EXPOSURE_BIN_COUNT];
} soc_auto_exposure;

/* --- Library / ABI introspection ---------------------------------------------------------------- */
int32_t soc_abi_version(void);
size_t soc_abi_sizeof(const char* type_name);                        /* "soc_globals", "soc_img", ... */
int64_t soc_abi_offsetof(const char* type_name, const char* field);  /* -1 if unknown */
const char* soc_last_error_string(void);
/* Tuning knobs (SOC_* environment variables of the profiling variants) are read once and cached;
 * this drops the cache so the current environment applies to the next launches. */
void soc_tuning_reload(void);
const char* soc_device_arch(void);                                   /* "gfx950" the kernels were built for */
/* Launch geometry (no GPU needed): SOC_OK when a block of bx x by x bz lanes fits a kernel whose flat work-group bound
 * (__launch_bounds__) is `bound`, else SOC_E_INVALID_ARG with the reason. Every launcher in the library applies the
 * same check with its kernel's own bound before the launch, so a block over the bound is never issued (it would fail
 * on the device as an "unspecified launch failure"). */
int soc_check_block_shape(int32_t bound, int32_t bx, int32_t by, int32_t bz);

/* --- Host-side globals feed (native C++, no GPU needed) ----------------------------------------- */
/* Renderer defaults: renderer.cpp:72-133 (terrain, ssao, composition, dof, auto exposure incl. the
 * log_min/log_max re-derivation of :103-104, tone mapping, sun ortho/lookAt/dir of :109-133). */
int soc_globals_init_defaults(soc_globals* g, int32_t width, int32_t height);

/* Camera state of ControlledCamera3D (camera.hpp:105-119): position + rotation (x = yaw, y = pitch). */
typedef struct soc_camera {
    float position[3];
    float rotation[3];
    float fov_degrees;   /* Camera3D::fov  = 90  (camera.hpp:74) */
    float near_clip;     /* Camera3D::near = 0.1 */
    float far_clip;      /* Camera3D::far  = 1000 */
} soc_camera;

/* One Application::update() (application.cpp:109-165) without input: rebuilds the camera view
 * (camera.cpp:40-56) and projection (camera.cpp:6-10, Y flip), the R2 jitter (period 32, :113-127,
 * applied to proj[3][0..1], :129-131), shifts current -> previous matrices, and advances
 * delta_time / elapsed_time / frame_counter. *jitter_index is advanced like the reference's. */
int soc_globals_frame_update(soc_globals* g, const soc_camera* cam, int32_t width, int32_t height,
                             float delta_time, uint32_t* jitter_index);

/* ECS scene feed: Scene::update (src/ecs/scene.cpp:47-118). An entity carries a TransformComponent (position,
 * rotation in degrees, scale; components.hpp) and optionally a PointLightComponent or SpotLightComponent
 * (color, intensity, cut_off / outer_cut_off in degrees; defaults components.hpp:55-66). soc_scene_update
 * clears the light counts, then walks the entities in order: every transform gets model = translate(position) *
 * toMat4(quat(radians(rotation))) * scale(scale) and normal = transpose(inverse(model)) (:64-68); a point light
 * appends {position, color, intensity}; a spot light appends {position, dir = rotateZ(rotateY(rotateX((0,-1,0),
 * rx), ry), rz), color, intensity, cos(radians(cut_off)), cos(radians(outer_cut_off))} (:87-116). More than
 * SOC_MAX_POINT_LIGHTS / SOC_MAX_SPOT_LIGHTS lights (an out-of-bounds write in the reference) is an error. */
#define SOC_ENTITY_POINT_LIGHT 1
#define SOC_ENTITY_SPOT_LIGHT 2
typedef struct soc_entity {
    float position[3];
    float rotation[3];       /* degrees */
    float scale[3];
    int32_t components;      /* SOC_ENTITY_* (a transform is always present) */
    float color[3];
    float intensity;
    float cut_off, outer_cut_off;   /* degrees (spot lights) */
} soc_entity;
/* model_matrices / normal_matrices: optional outputs, count x float[16] (column-major), or NULL. */
int soc_scene_update(soc_globals* g, const soc_entity* entities, int32_t count, float* model_matrices,
                     float* normal_matrices);

/* glm restatements used by the feed (exported for tests): column-major float[16]. */
void soc_mat4_perspective_rh_no(float out[16], float fovy_radians, float aspect, float znear, float zfar);
void soc_mat4_ortho_rh_no(float out[16], float l, float r, float b, float t, float znear, float zfar);
void soc_mat4_look_at_rh(float out[16], const float eye[3], const float center[3], const float up[3]);
void soc_mat4_inverse(float out[16], const float m[16]);
void soc_mat4_mul(float out[16], const float a[16], const float b[16]);

/* --- ★ Passes (one per reference task) ---------------------------------------------------------- */

/* BloomDownsampleTask (src/graphics/tasks/bloom_downsample.inl:19-68, shader :107-141):
 * 13-tap COD:AW filter of `higher_mip` written to `lower_mip` (any size ratio; exact 1:1 and 2:1
 * fast paths). RGBA16F -> RGBA16F. */
int soc_bloom_downsample(const soc_globals* g, soc_img higher_mip, soc_img lower_mip, soc_stream stream);

/* BloomUpsampleTask (bloom_upsample.inl:19-77, shader :98-127): 9-tap tent of `lower_mip` that
 * OVERWRITES `higher_mip` (CLEAR + ONE/ONE blend == overwrite, quirk Q5). RGBA16F -> RGBA16F. */
int soc_bloom_upsample(const soc_globals* g, soc_img lower_mip, soc_img higher_mip, soc_stream stream);

/* Whole bloom chain as scheduled by renderer.cpp:1024-1062: down(emissive->mip0), down(mip i ->
 * mip i+1), up(mip i -> mip i-1), up(mip0 -> emissive). `mips` holds mip_count images (4 in the
 * reference, renderer.hpp:51). The reference's 8 passes, bit-exact. */
int soc_bloom_chain(const soc_globals* g, soc_img emissive, const soc_img* mips, int32_t mip_count,
                    soc_stream stream);

/* The bloom chain in weighted form (bloom_w.hip): at the chain's fixed ratios every tap of the sampling
 * contract has exact weights on clamp-to-edge texels, so each pass is evaluated as one fixed weighted
 * sum of RGBA16F texels with fp32 FMAs (same weights, different rounding order: within the RGBA16F
 * tolerance, not bit-exact). Stages: 1 emissive -> [mip0] -> mips[1], 2 mips[1] -> [mip2] -> mips[3],
 * 3 mips[3] -> [mip2] -> mips[1], 4 mips[1] -> [mip0] -> output; 0 = all four. mips[0] and mips[2] are
 * scratch (never written: their final contents are unobservable in the reference graph). Needs 4 mips halving
 * exactly from the emissive extent (<= 8192); output may be `emissive` (in place, as the reference) but not mips[1]. */
int soc_bloom_weighted_stage(const soc_globals* g, soc_img emissive, const soc_img* mips, int32_t mip_count, soc_img output,
                             int32_t stage, soc_stream stream);

/* SSAOGenerationTask (ssao_generation.inl:20-68, shader :176-214): half-res R8 ambient occlusion from
 * full-res depth (D32F) and normal (RGBA16F). `target` is (W/2)x(H/2) R8_UNORM. `noise_table` is an
 * optional device workspace of (target.w * target.h * 2) floats holding the per-pixel random vector
 * of :184-188 (a pure function of uv and the normal-image size, filled by
 * soc_ssao_prepare_noise); pass NULL to evaluate it inline. */
int soc_ssao_prepare_noise(soc_img normal, soc_img target, float* noise_table, soc_stream stream);
int soc_ssao_generation(const soc_globals* g, soc_img depth, soc_img normal, soc_img target,
                        const float* noise_table, soc_stream stream);

/* SSAOBlurTask (ssao_blur.inl:19-70, shader :91-106): 4x4 box, offsets -2..+1. R8 -> R8. */
int soc_ssao_blur(const soc_globals* g, soc_img ssao, soc_img target, soc_stream stream);

/* ScreenSpaceReflectionTask (screen_space_reflection.inl:26-70, shader :88-183): per pixel, a pixel whose
 * metallic_roughness.y is below 0.01 copies its albedo; every other pixel reflects its view ray about the view-space
 * normal and marches it through `depth` (up to 50 probes: a growing step until the ray passes behind the depth image,
 * then a binary search), writing the albedo at the probe that comes within 0.05 of the depth image, or (0, 0, 0, 1)
 * when none does (quirk Q13: the shader's fallback to the pixel's own albedo cannot fire). depth: D32F; normal, albedo,
 * metallic_roughness, target: RGBA16F; all of the target's extent (at most 8192 x 8192). `steps` (optional, data NULL =
 * none): R8 of the same extent, the raw byte per pixel: 0..49 the iteration of the hit, 50 a miss, 255 a copied pixel;
 * the colours are the same bits with or without it. The reference runs the task every frame between SSAOBlur and
 * CloudRendering (renderer.cpp:1081-1092) although nothing reads its image (composition.inl:213-216 is commented out);
 * here it is opt-in: the default render graph does not run it (soc_renderer_add_screen_space_reflection). */
int soc_screen_space_reflection(const soc_globals* g, soc_img depth, soc_img normal, soc_img albedo,
                                soc_img metallic_roughness, soc_img target, soc_img steps /* data NULL = none */,
                                soc_stream stream);

/* The reference's depth-of-field task chain (depth_of_field.inl; its three add_task calls are commented out,
 * renderer.cpp:1119-1153). Here it is opt-in: the default render graph does not run it (soc_renderer_add_depth_of_field).
 *
 * The chain is depth_of_field_image (renderer.cpp:346, 463-468): RGBA16F, floor(log2(max(W, H))) + 1 levels, level k of
 * max(1, W >> k) x max(1, H >> k) texels, in soc_generate_mips's packed layout at 8 B per texel: level 0 at
 * pitch_bytes (at least 8 W, a multiple of 8), level k >= 1 at data + pitch_bytes * H + sum_{1 <= j < k} 8 w_j h_j with
 * tight rows. soc_depth_of_field_chain_bytes is the size of the whole allocation (0 for bad arguments: an extent
 * outside 1..8192, a pitch below 8 W or no multiple of 8). */
size_t soc_depth_of_field_chain_bytes(int32_t width, int32_t height, int32_t pitch_bytes);
/* BlitImageToImage (depth_of_field.inl:16-48) and every MipMapping - i (:55-88, renderer.cpp:1127-1144): level 0 of
 * `chain` becomes a bit copy of `color`, level k a LINEAR blit (vkCmdBlitImage) of level k - 1 with soc_generate_mips's
 * taps and 8-bit weights, filtered in f32 and rounded to f16 nearest-even. `chain` is the RGBA16F view of level 0; its
 * allocation is soc_depth_of_field_chain_bytes(width, height, pitch_bytes) long. color: RGBA16F of the same extent
 * (at most 8192 x 8192) that does not overlap the chain's allocation. */
int soc_depth_of_field_mips(soc_img color, soc_img chain, soc_stream stream);
/* DepthOfFieldTask (depth_of_field.inl:104-155, shader :176-199): a pixel with depth < 1 becomes the mean of four
 * textureGrad taps of the chain at uv +- (1 / W, 0) and uv +- (0, 1 / H), both gradients (c, c) with c = coc / max_coc
 * from g's camera clips, focal_length, plane_in_focus and aperture, through depth_of_field_sampler (renderer.cpp:472-488:
 * trilinear, REPEAT, max_lod past the last level), with alpha 1; any other pixel (NaN depth included) is the chain's
 * level-0 texel, alpha kept (quirk Q14). depth: D32F; chain: as soc_depth_of_field_mips left it; target: RGBA16F; all of
 * one extent. The target is never read, so it may be the image the chain was built from (the reference's arrangement:
 * color_image); it may not overlap the chain's allocation (SOC_E_INVALID_ARG, "alias"). */
int soc_depth_of_field(const soc_globals* g, soc_img depth, soc_img chain, soc_img target, soc_stream stream);

/* CloudRenderingTask (cloud_rendering.inl:27-54, shader :441-481): atmosphere + volumetric clouds on
 * sky pixels (depth == 1), constant (0.2,0.4,1.0) elsewhere. `noise` is the 64x64 RGBA8 or R8
 * noise texture (assets/Clouds/noise.png, REPEAT). target: RGBA8_UNORM full-res (quirk Q6).
 * `workspace` (optional, soc_cloud_rendering_workspace_size(target.width, target.height) bytes of
 * device memory) enables the compacted path: sky pixels are listed, and the cloud march is split at
 * its dense steps into (pixel, step) pairs so the sun-visibility marches are spread evenly over the
 * lanes; the result is bit-identical to the workspace-free single kernel. The call is stateless: it builds its
 * tables in the workspace (secondary-ray optical depths, noise quads) from this call's sun and noise on every call, and
 * assumes nothing about what the workspace held before. A workspace given to a renderer (soc_frame_images) belongs to
 * it between frames: see soc_renderer_invalidate_cloud_tables. */
size_t soc_cloud_rendering_workspace_size(int32_t width, int32_t height);
int soc_cloud_rendering(const soc_globals* g, soc_img depth, soc_img noise, soc_img target, void* workspace,
                        soc_stream stream);

/* CompositionTask (composition.inl:29-79, shader :162-225): deferred lighting with the sun ESM
 * shadow, point/spot lights, ambient * AO^strength, emissive * strength, clouds on sky pixels.
 * `d_globals` is a DEVICE copy of *g (soc_upload_globals) and is only read when the frame has
 * point or spot lights (it may be NULL otherwise). Writes RGBA16F `target`. */
int soc_composition(const soc_globals* g, const soc_globals* d_globals, soc_img target, soc_img albedo,
                    soc_img emissive, soc_img normal, soc_img depth, soc_img ssao, soc_img shadow,
                    soc_img clouds, soc_stream stream);

/* CompositionTask followed by GenerateLuminanceHistogramTask (renderer.cpp:1103-1168) in one launch
 * when the composition pair path applies at g->resolution: the bins of the stored RGBA16F pixels are
 * accumulated while they are written (bit-identical bins, no re-read of `target`). Otherwise the two
 * passes run back to back. The bins are ADDED to ae->histogram_buckets, as the histogram pass does.
 * `scratch`: device, SOC_HISTOGRAM_SCRATCH_WORDS u32, zero-filled by the caller once; every call leaves
 * it zeroed again (8 partial histograms, folded into the bins by a second small launch). */
#define SOC_HISTOGRAM_SCRATCH_WORDS 2048
int soc_composition_luminance_histogram(const soc_globals* g, const soc_globals* d_globals, soc_img target,
                                        soc_img albedo, soc_img emissive, soc_img normal, soc_img depth,
                                        soc_img ssao, soc_img shadow, soc_img clouds, soc_auto_exposure* d_auto_exposure,
                                        uint32_t* scratch, soc_stream stream);

/* GenerateLuminanceHistogramTask (generate_luminance_histogram.inl:23-47, shader :59-78): adds the
 * frame's 256-bin log-luminance histogram into d_auto_exposure->histogram_buckets. */
int soc_generate_luminance_histogram(const soc_globals* g, soc_img hdr, soc_auto_exposure* d_auto_exposure,
                                     soc_stream stream);

/* ResolveLuminanceHistogramTask (resolve_luminance_histogram.inl:20-43, shader :56-80): weighted mean
 * of the bins -> exposure (exponential adaptation), then clears the bins.
 * total_pixels == 0 -> resolution.x*resolution.y (reference). wide_accumulator != 0 -> 64-bit
 * weighted sum (multi-GPU all-reduced bins); 0 -> reference u32 wrap semantics. */
int soc_resolve_luminance_histogram(const soc_globals* g, soc_auto_exposure* d_auto_exposure,
                                    uint64_t total_pixels, int32_t wide_accumulator, soc_stream stream);

/* TemporalAntiAliasingTask (temporal_antialiasing.inl:54-116, shader :137-190). Writes RGBA16F
 * `target`. If `velocity_history_out` has data != NULL, the kernel also writes a copy of
 * current_velocity into it (fused CopyImageTask of renderer.cpp:1191-1198); it must not alias
 * previous_velocity. */
int soc_temporal_antialiasing(const soc_globals* g, soc_img target, soc_img current_color,
                              soc_img previous_color, soc_img current_velocity, soc_img previous_velocity,
                              soc_img depth, soc_img velocity_history_out, soc_stream stream);

/* TemporalAntiAliasingTask followed by ToneMappingTask (renderer.cpp:1170-1217) in one launch when
 * `output` is RGBA8_UNORM at the target extent and the TAA pair path applies: the resolved RGBA16F
 * pixels are tone-mapped as stored (same AgX device code as soc_tone_mapping), saving the re-read of
 * `target`. Otherwise the two passes run back to back. Results equal soc_temporal_antialiasing +
 * soc_tone_mapping. */
int soc_temporal_antialiasing_tone_mapping(const soc_globals* g, soc_img target, soc_img current_color,
                                           soc_img previous_color, soc_img current_velocity,
                                           soc_img previous_velocity, soc_img depth, soc_img velocity_history_out,
                                           const soc_auto_exposure* d_auto_exposure, soc_img output,
                                           soc_stream stream);

/* CopyImageTask (temporal_antialiasing.inl:16-37): same-format, same-extent image copy. */
int soc_copy_image(soc_img target, soc_img source, soc_stream stream);

/* ToneMappingTask (tone_mapping.inl:20-70, shader :145-176): AgX-DS with exposure from
 * d_auto_exposure->exposure. target: RGBA8_UNORM / RGBA8_SRGB / RGBA16F / RGBA32F. */
int soc_tone_mapping(const soc_globals* g, soc_img color, const soc_auto_exposure* d_auto_exposure,
                     soc_img target, soc_stream stream);

/* Device copy of the globals block (the reference's per-frame UBO upload, renderer.cpp:648-657). */
int soc_upload_globals(const soc_globals* g, soc_globals* d_globals, soc_stream stream);

/* --- Bounded lights (opt-in) ------------------------------------------------------
 * The reference's lights reach everywhere (1/d^2 never ends), so every pixel pays for every light. A caller may give
 * each light a range r (0: unlimited, as the reference; else finite and > 0), indexed like the globals' point_lights /
 * spot_lights (soc_scene_update appends the lights in entity order per kind). A ranged light's contribution is
 * multiplied by w = clamp(1 - (d^2 / r^2)^2, 0, 1) (KHR_lights_punctual's window), and with f = w for a point light,
 * f = w * the cone term for a spot light (the cone term alone for an unlimited one), a light contributes to a pixel
 * only where f > 0: elsewhere it contributes nothing, a NaN or Inf term included (the unbounded calls add NaN * 0
 * outside a spot's cone where the normal is not unit). An unlimited point light is exactly the unbounded one: a
 * bounded call whose ranges are all 0 and which has no spot lights gives soc_composition's bits.
 * A range so large that 1 / r^2 is below fp32 acts as unlimited; one so small that it is above fp32 is clamped. */
typedef struct soc_light_bounds {
    float point_range[SOC_MAX_POINT_LIGHTS];
    float spot_range[SOC_MAX_SPOT_LIGHTS];
} soc_light_bounds;
/* Bytes of the DEVICE record the bounded kernels read (the library's own layout, not soc_light_bounds). */
#define SOC_LIGHT_BOUNDS_DEVICE_BYTES 2048
/* Validates every range (negative, NaN or Inf: SOC_E_INVALID_ARG naming the first bad index, before any HIP call),
 * then writes the device record to d_bounds, stream-ordered like soc_upload_globals (the host struct is consumed
 * before the call returns). */
int soc_upload_light_bounds(const soc_light_bounds* host, void* d_bounds, soc_stream stream);
/* SOC_LIGHTS_CULL: on the pair path each wave tests the lights against the box of its 16x8 patch's lit pixels first and
 * runs its loops over the lights that may reach it; the result is bit-identical to the call without the flag (the test
 * is conservative against the per-pixel test as the device computes it, csrc/light_cull.hpp). Ignored off the pair
 * path (odd widths, misaligned views). */
#define SOC_LIGHTS_CULL 1u
/* soc_composition / soc_composition_luminance_histogram with bounded lights. d_bounds (soc_upload_light_bounds) must not
 * be NULL. d_shaded_pairs (device u32, may be NULL; measuring only: it selects kernels that pay one atomic per wave):
 * on the pair path every wave with a lit pixel adds the number of lights its loops ran (all of them without
 * SOC_LIGHTS_CULL); untouched off the pair path. */
int soc_composition_bounded(const soc_globals* g, const soc_globals* d_globals, soc_img target, soc_img albedo,
                            soc_img emissive, soc_img normal, soc_img depth, soc_img ssao, soc_img shadow,
                            soc_img clouds, const void* d_bounds, uint32_t flags, uint32_t* d_shaded_pairs,
                            soc_stream stream);
int soc_composition_luminance_histogram_bounded(const soc_globals* g, const soc_globals* d_globals, soc_img target,
                                                soc_img albedo, soc_img emissive, soc_img normal, soc_img depth,
                                                soc_img ssao, soc_img shadow, soc_img clouds,
                                                soc_auto_exposure* d_auto_exposure, uint32_t* scratch,
                                                const void* d_bounds, uint32_t flags, uint32_t* d_shaded_pairs,
                                                soc_stream stream);

/* --- Cascaded sun shadow maps (opt-in) ---------------------------------------------
 * The reference has one fixed orthographic ESM map (sun_info.projection_view_matrix). A caller may instead give
 * Composition up to four maps fitted to slices of the camera's frustum, stacked vertically in ONE D32F atlas: cascade k
 * is rows [k * map_size, (k + 1) * map_size) of a map_size x (count * map_size) image.
 * A lit pixel uses cascade k = the number of i < count - 1 with depth > split_depth[i], compared on the stored float32
 * depth (a NaN depth: cascade 0; a pixel beyond the last split still samples the last cascade, clamped). The shadow term
 * is the reference's per cascade: project with projection_view[k], one bilinear tap at xy * 0.5 + 0.5 inside slab k
 * (clamp-to-edge never reads a neighbouring slab), then clamp(pow(exp(exponential_factor[k] * (z - d)),
 * sun_info.darkening_factor), 0, 1). No blending between cascades.
 * The fitted cascades keep the sun's softness in world units, so their factors are large (-1000 .. -2500 for slices
 * 50 - 200 units wide); the cascaded kernels therefore compute a pixel's sun-space position and tap coordinate in fp64
 * (from the same fp32 matrices, depth and pixel centre), which soc_composition's fp32 arithmetic cannot hold to the
 * RGBA16F tolerance at such factors. */
#define SOC_MAX_SUN_CASCADES 4
typedef struct soc_sun_cascades {
    int32_t count;                  /* 1..4 */
    int32_t map_size;               /* S: cascade k is rows [k*S, (k+1)*S) of an S x (count*S) D32F atlas */
    float projection_view[4][16];   /* column-major, as sun_info.projection_view_matrix */
    float split_depth[4];           /* depth-buffer values, strictly increasing; [count-1..] unused */
    float exponential_factor[4];    /* ESM factor per cascade */
} soc_sun_cascades;
/* The one-cascade record of the globals' own sun: projection_matrix * view_matrix in host fp32 and the sun's factor. A
 * cascaded call with it and the S x S map computes soc_composition's term with the fp64 position: the same bits wherever
 * the two roundings of the term agree (all of them on the test frames; 94 of 8.3 M pixels differ by one RGBA16F step at
 * 3840x2160 on the C4 terrain), not by construction. No HIP call. */
int soc_sun_cascades_from_sun(const soc_globals* g, int32_t map_size, soc_sun_cascades* out);
/* Fits `count` cascades to the camera's unjittered frustum between near_distance and max_distance (view distances).
 * Slice far distances: d_i = lambda n (f/n)^(i/N) + (1 - lambda)(n + (f - n) i/N); split_depth[i] is the depth-buffer
 * value of a view-axis point at d_(i+1). Per slice: the bounding sphere of its eight corners, radius rounded up to a
 * multiple of 1/8 world unit (the extent does not change when the camera only rotates), centre snapped to whole shadow
 * texels (2r / map_size) in light space, lookAt along sun_info.direction with up (0, -1, 0), an orthographic projection
 * whose depth range holds the sphere and anything up to caster_margin world units towards the sun in z_ndc [0, 1].
 * exponential_factor[k] = sun_info.exponential_factor * P_sun[10] / P_k[10]: the sun's softness in world units.
 * SOC_E_INVALID_ARG (naming the argument) for count outside 1..4, map_size < 2, split_lambda outside [0, 1], not
 * 0 < near_distance < max_distance, a negative margin or a non-finite value. No HIP call. */
int soc_sun_cascades_fit(const soc_globals* g, int32_t count, int32_t map_size, float near_distance, float max_distance,
                         float split_lambda, float caster_margin, soc_sun_cascades* out);
/* soc_composition / soc_composition_luminance_histogram with `shadow` = the cascades' atlas. The record is host memory,
 * consumed before the call returns. Validated before any HIP call (SOC_E_INVALID_ARG naming the field: count, map_size,
 * the atlas extent or format, split_depth, exponential_factor, projection_view). */
int soc_composition_cascaded(const soc_globals* g, const soc_globals* d_globals, soc_img target, soc_img albedo,
                             soc_img emissive, soc_img normal, soc_img depth, soc_img ssao, soc_img shadow,
                             soc_img clouds, const soc_sun_cascades* cascades, soc_stream stream);
int soc_composition_luminance_histogram_cascaded(const soc_globals* g, const soc_globals* d_globals, soc_img target,
                                                 soc_img albedo, soc_img emissive, soc_img normal, soc_img depth,
                                                 soc_img ssao, soc_img shadow, soc_img clouds,
                                                 soc_auto_exposure* d_auto_exposure, uint32_t* scratch,
                                                 const soc_sun_cascades* cascades, soc_stream stream);

/* --- Render graph (host C++ mirror of Renderer::rebuild_task_graph, renderer.cpp:929-1235) ------ */

/* Frame images. The caller allocates them (device memory) and keeps them alive. */
typedef struct soc_frame_images {
    soc_img albedo, emissive, normal, depth, velocity;  /* G-buffer (produced upstream) */
    soc_img shadow;                                     /* sun shadow map, D32F 4096^2 */
    soc_img noise;                                      /* clouds noise 64^2 */
    soc_img bloom_mips[4];                              /* RGBA16F W,W/2,W/4,W/8 */
    soc_img ssao, ssao_blur;                            /* R8 (W/2)x(H/2) */
    soc_img clouds;                                     /* RGBA8 WxH */
    soc_img color;                                      /* RGBA16F composition output */
    soc_img history_color[2];                           /* RGBA16F TAA resolved / previous (ping-pong) */
    soc_img history_velocity[2];                        /* RGBA16F previous velocity (ping-pong) */
    soc_img output;                                     /* tone-mapped framebuffer (RGBA8) */
    float* ssao_noise_table;                            /* optional (ssao.w*ssao.h*2 floats) or NULL */
    soc_auto_exposure* auto_exposure;                   /* device */
    soc_globals* d_globals;                             /* device copy of the globals */
    /* Optional target of the last bloom upsample, read by composition as "emissive". data == NULL:
     * bloom overwrites `emissive` in place, as the reference graph does (renderer.cpp:1055-1062). */
    soc_img bloom_output;
    void* clouds_workspace;                             /* optional, soc_cloud_rendering_workspace_size */
} soc_frame_images;

typedef struct soc_renderer soc_renderer;

/* Phases of one frame. The luminance all-reduce of a multi-GPU run sits between PRE and POST. */
#define SOC_PHASE_PRE_EXPOSURE 1   /* bloom, ssao, blur, clouds, composition, histogram */
#define SOC_PHASE_POST_EXPOSURE 2  /* resolve, taa (+ fused velocity history), tone mapping */
#define SOC_PHASE_ALL 3

/* flags */
#define SOC_RENDERER_TIMING 1      /* record hipEvents around every pass (GPUMetric, gpu_metric.cpp:18-42) */
#define SOC_RENDERER_UNFUSED_BLOOM 2  /* bloom as the reference's 8 bit-exact passes (as EXACT_BLOOM) */
#define SOC_RENDERER_SERIAL 4      /* every pass on the caller's stream (no concurrent sky lane) */
#define SOC_RENDERER_UNFUSED_TONEMAP 8  /* TAA and tone mapping as two passes (default: one launch for RGBA8) */
#define SOC_RENDERER_FUSED_HISTOGRAM 16  /* composition + luminance histogram in one launch (the default; kept
                                            for callers that set it) */
#define SOC_RENDERER_EXACT_BLOOM 32       /* bit-exact 8-pass bloom chain instead of the weighted form (bloom_w.hip) */
#define SOC_RENDERER_UNFUSED_HISTOGRAM 64 /* composition and luminance histogram as two passes */
#define SOC_RENDERER_NO_SKY_SPLIT 128     /* Composition writes the sky pixels itself (waits for the clouds) */
/* The caller does not rewrite the frame's input images (G-buffer, shadow map, noise) between frames, e.g. a resident
 * G-buffer, or one produced in the graph by the raster head. Second-lane passes whose only cross-frame dependencies are
 * on the second lane (CloudRendering: it writes only CLOUDS) may then start before the fork, i.e. before the caller's
 * stream reaches this frame: the clouds of frame N+1 overlap the composition / TAA of frame N. Same results. The
 * second lane's intermediate CLOUDS image may then already hold the next frame's clouds when work the caller queued
 * between two calls reads it: a caller that reads CLOUDS between frames leaves the flag off. The transform array of a
 * draw scene (soc_renderer_set_draw_scene) is not such an input image: its readers (DepthPrepass and GBufferGeneration
 * on the caller's stream, SunShadowDraw on the second lane, which has a ring edge on the previous frame's Composition
 * and so always waits for the fork) follow everything the caller queued before the call, so the caller may rewrite
 * it on its stream between frames with the flag set. */
#define SOC_RENDERER_STATIC_INPUTS 256
/* Velocity history by slot rotation instead of a copy. The reference copies the velocity image into
 * previous_velocity after TAA every frame (CopyImageTask, renderer.cpp:1185-1189; without this flag the TAA launch
 * writes that copy into the history_velocity slot it resolves into). With the flag, the frame's velocity image IS that
 * slot: the velocity producer (GBufferGeneration of the raster head, or the caller) writes frame N's velocity into
 * history_velocity[1 - soc_renderer_current_history(r)] (read before executing frame N), TAA reads it there and frame
 * N + 1 reads it as its previous velocity, so no copy is made. images.velocity is then unused; caller passes receive the
 * slot as `images->velocity`, and VELOCITY / PREVIOUS_VELOCITY declared by a pass count as uses of both slots. Same
 * results as the copy for the same velocity fields. */
#define SOC_RENDERER_VELOCITY_SLOTS 512
/* The bloom chain's last stage (upsample 1 + 0: mip1 -> [mip0] -> bloom output, renderer.cpp:1044-1062) may be computed
 * inside the fused Composition + histogram launch, per 32 x 16 tile in LDS, from BLOOM_MIP1 (the same values per pixel,
 * rounded to RGBA16F as the chain stores them, so the same colour bits). The renderer does so in frames whose sky lane
 * is the critical path (a high-priority sky lane: soc_renderer_side_queue() == 1, and the lane probe's high-priority
 * windows); the chain's fourth pass then records nothing and the
 * full-resolution bloom output (images.bloom_output, or the emissive image in place) is NOT written. Composition
 * declares BLOOM_MIP1 and BLOOM_MIP3 besides the bloom output. Applies with the weighted chain and the fused histogram's
 * pair path. A caller that reads the bloom output leaves the flag off.
 * In the other frames of such a renderer (a low-priority sky lane) the fourth pass runs, but SPARSE: the chain's output
 * is a function of BLOOM_MIP3 alone, and where the mip3 texels that reach an aligned 32 x 16 output cell all have the
 * bit pattern 0x0000 in their RGB halves, the cell is (+0, +0, +0, 1) whichever kernel computes it. The fourth pass
 * stores nothing in a 62 x 16 strip whose cells are all such, and Composition tests the same cells on the same mip3 and
 * takes the constant there instead of loading the bloom output, so the colour bits are the same and the bloom output
 * keeps stale or unwritten pixels in those cells. Only when Composition is the one pass of the graph that declares
 * BLOOM_OUTPUT (a caller's pass that reads or writes it gets every pixel written), images.bloom_output is set, and the
 * frame's Composition takes the pair path; SOC_BLOOM_SPARSE=0 (tuning knob) writes and loads every pixel.
 * soc_bloom_weighted_stage itself always writes its whole output. */
#define SOC_RENDERER_BLOOM_IN_COMPOSITION 1024
/* The sky lane's hardware queue (soc_renderer_side_queue): a low-priority stream by default (frames whose main lane is
 * the critical path, e.g. the Sponza frames at 4K); SOC_RENDERER_SKY_LANE_HIGH a high-priority stream (sky-bound frames:
 * the terrain / 1080p frames), which also selects the sky-bound variants (BLOOM_IN_COMPOSITION, the clouds' density grid
 * at twice the resident set, hoisted classification); SOC_RENDERER_SKY_LANE_PROBE times both over the first frames and
 * keeps the faster (round 5's default; the choice can then differ between runs). Same results in every case. */
#define SOC_RENDERER_SKY_LANE_HIGH 2048
#define SOC_RENDERER_SKY_LANE_PROBE 4096

soc_renderer* soc_renderer_create(const soc_frame_images* images, uint32_t flags);
void soc_renderer_destroy(soc_renderer* r);
int soc_renderer_execute(soc_renderer* r, const soc_globals* g, int32_t phase, soc_stream stream);
/* Histogram normalisation for a multi-GPU resolve: total pixels over all ranks (0 = this frame). */
int soc_renderer_set_exposure_pixels(soc_renderer* r, uint64_t total_pixels, int32_t wide_accumulator);
/* Composition with bounded lights (above) in either histogram mode: d_bounds is the device record the caller rewrites
 * between frames on its stream (soc_upload_light_bounds), like every frame input; flags: SOC_LIGHTS_*. NULL removes
 * the setting. The pass's declared uses, the graph and the frame plan are unchanged. */
int soc_renderer_set_light_bounds(soc_renderer* r, const void* d_bounds, uint32_t flags);
/* Cascaded sun shadows (above): the record is copied (no HIP call; a caller refits and sets it every frame the camera
 * moves) and images.shadow must be its atlas (checked here and again at execute). While set, SunShadowDraw and
 * SunShadowDrawTerrain draw every cascade into its slab within their pass (names, lanes and the frame plan unchanged)
 * and Composition launches the cascaded call. NULL: back to the one map. Together with soc_renderer_set_light_bounds,
 * SOC_RENDERER_BLOOM_IN_COMPOSITION or the bloom's zero cells: SOC_E_UNSUPPORTED naming the pair. */
int soc_renderer_set_sun_cascades(soc_renderer* r, const soc_sun_cascades* cascades);
int32_t soc_renderer_pass_count(const soc_renderer* r);
const char* soc_renderer_pass_name(const soc_renderer* r, int32_t index);
const char* soc_renderer_pass_group(const soc_renderer* r, int32_t index);   /* renderer.cpp:558-588 names */
/* Milliseconds of pass `index` in the most recent executed frame (needs timing enabled for the pass
 * and a completed stream); < 0 if unavailable. */
float soc_renderer_pass_ms(soc_renderer* r, int32_t index);
/* Per-pass timing control: hipEvents bracket a timed pass on the launch stream every frame, kept in
 * a ring of SOC_RENDERER_TIMING_RING frames. index -1 = every pass. Event creation happens here, not
 * in soc_renderer_execute. */
#define SOC_RENDERER_TIMING_RING 256
int soc_renderer_set_pass_timing(soc_renderer* r, int32_t index, int32_t enable);
int soc_renderer_reset_timing(soc_renderer* r);
/* Sum of the pass's durations (ms) over the frames recorded since the last reset (at most the last
 * SOC_RENDERER_TIMING_RING) and their count. Needs a completed stream. */
int soc_renderer_pass_stats(soc_renderer* r, int32_t index, float* total_ms, int32_t* frames);
/* The recorded frames' start / end event times of the pass (ms after the caller's hipEvent `base`, recorded on the same
 * device before them), oldest first; at most n entries; returns the count written or < 0. Needs a completed stream.
 * For checking the pass events against a kernel trace of the same run (tools/event_trace_check.py). */
int32_t soc_renderer_pass_event_times(soc_renderer* r, int32_t index, void* base, float* start_ms, float* end_ms,
                                      int32_t n);
/* Index (0/1) of the history_color slot holding this frame's TAA result (= tone-map input). */
int32_t soc_renderer_current_history(const soc_renderer* r);
/* Restore that index when resuming from a checkpoint of the temporal state (SURVEY.md §5 "Checkpoint / resume"; the
 * reference keeps it only in its TAA history images and AutoExposure, renderer.cpp:1170-1198): the caller writes back
 * history_color[index] / history_velocity[index] and the AutoExposure block, then sets the index. 0 or 1. */
int soc_renderer_set_current_history(soc_renderer* r, int32_t index);
/* Sky lane on/off (default on unless SOC_RENDERER_SERIAL). On: CloudRendering runs on a renderer-owned
 * stream of the current device, forked from `stream` at the start of the PRE phase and joined before
 * Composition, so it overlaps bloom and SSAO. Results are identical either way. */
int soc_renderer_set_async(soc_renderer* r, int32_t enable);
/* The renderer's CloudRendering keeps two static tables in images.clouds_workspace between frames: the secondary-ray
 * optical-depth table, rebuilt when the bit pattern of dot(sun, sun) of the globals' sun direction changes, and the
 * noise quad tables, rebuilt when the noise image's data pointer, format or pitch changes. A caller that rewrites the
 * noise texels IN PLACE, or that uses the workspace for anything else between two frames (soc_cloud_rendering included),
 * calls this before the next soc_renderer_execute: the next frame rebuilds both tables and clears the workspace's
 * counter blocks. Host-side only (no launch, no synchronisation). */
int soc_renderer_invalidate_cloud_tables(soc_renderer* r);
/* The sky lane's hardware queue: 1 = a high-priority stream, 2 = low priority, 0 = normal priority (a queue HIP may
 * share with the caller's stream), -1 = not chosen yet (SOC_RENDERER_SKY_LANE_PROBE: after 16 frames, eight windows of
 * 32-128 frames alternate high / low priority as ABBA pairs; high is kept if it is faster by more than 2 % once their
 * timing events have completed, else low) or no sky lane created. Same results either way. */
int32_t soc_renderer_side_queue(const soc_renderer* r);
/* Frames the auto probe spans from the renderer's first call (the choice is made at the first call after they have
 * completed on the GPU); 0 when no probe runs. A caller that times frames runs at least this many first. */
int32_t soc_renderer_side_queue_probe_frames(const soc_renderer* r);

/* --- Pass declaration (the Daxa task-uses block + TaskGraph::add_task, e.g. composition.inl:10-21 and
 * renderer.cpp:1103-1117) ------------------------------------------------------------------------
 * Every pass of the graph, built-in or added, declares the frame resources it reads and writes. The graph
 * keeps the registration order (the reference executes tasks in add_task order) and derives from the
 * declared uses what Daxa derives barriers from: each pass's dependencies (read-after-write,
 * write-after-read, write-after-write on the latest earlier user of a resource) and the placement of
 * SOC_PASS_ASYNC passes on the renderer's second lane: such a pass waits only for the passes it depends
 * on, and a later pass on the caller's stream waits for it only if it depends on it. */
enum soc_resource {
    SOC_RES_ALBEDO = 0, SOC_RES_EMISSIVE, SOC_RES_NORMAL, SOC_RES_DEPTH, SOC_RES_VELOCITY,
    SOC_RES_SUN_SHADOW, SOC_RES_NOISE,
    SOC_RES_BLOOM_MIP0, SOC_RES_BLOOM_MIP1, SOC_RES_BLOOM_MIP2, SOC_RES_BLOOM_MIP3,
    SOC_RES_BLOOM_OUTPUT,        /* images.bloom_output (aliases EMISSIVE when that image is absent) */
    SOC_RES_SSAO, SOC_RES_SSAO_BLUR, SOC_RES_CLOUDS, SOC_RES_COLOR,
    SOC_RES_PREVIOUS_COLOR, SOC_RES_RESOLVED,          /* TAA history pair, renderer.cpp:1170-1198 */
    SOC_RES_PREVIOUS_VELOCITY,
    SOC_RES_AUTO_EXPOSURE,       /* AutoExposure buffer (histogram bins + exposure) */
    SOC_RES_OUTPUT,              /* tone-mapped framebuffer (the reference's swapchain image) */
    SOC_RES_VISIBILITY,          /* raster visibility buffer (raster head) */
    SOC_RES_HISTOGRAM_PARTIALS,  /* the fused composition + histogram pass's partial bins */
    SOC_RES_SKY_COLOR,           /* the colour image's sky pixels, when the second lane writes them (see below) */
    SOC_RES_SKY_HISTOGRAM_PARTIALS,  /* their partial bins */
    SOC_RES_USER0 = 32,          /* SOC_RES_USER0 .. SOC_RES_USER0 + 31: caller-defined resources */
    SOC_RES_COUNT = 64
};
#define SOC_PASS_MAX_USES 16
#define SOC_PASS_ASYNC 1          /* may run on the second lane (the reference's unused async-compute queue) */
typedef struct soc_pass_desc {
    const char* name;             /* task name, unique in the graph */
    const char* group;            /* GPU-metric group (renderer.cpp:577-588) or any label */
    int32_t phase;                /* SOC_PHASE_PRE_EXPOSURE or SOC_PHASE_POST_EXPOSURE */
    uint32_t flags;               /* SOC_PASS_ASYNC */
    int32_t read_count, write_count;
    int32_t reads[SOC_PASS_MAX_USES];    /* enum soc_resource */
    int32_t writes[SOC_PASS_MAX_USES];
} soc_pass_desc;
/* Sky split (the default with the fused histogram and the pair path): Composition's sky pixels (depth == 1 ->
 * the clouds texel, composition.inl:220-222) are written and binned on the second lane right after
 * CloudRendering, so Composition does not wait for the clouds. COLOR is then the non-sky pixels and SKY_COLOR the
 * sky pixels of the same image: a caller pass that needs the whole colour image declares both.
 * SOC_RENDERER_NO_SKY_SPLIT turns it off (same bits either way). */
/* The callback of a caller pass: record its work on `stream`, return 0 (or a negative code, which aborts the
 * frame with that code). `images` is the renderer's frame, with history_color[0] / history_velocity[0] the
 * PREVIOUS and [1] the RESOLVED slots of this frame. */
typedef int32_t (*soc_pass_callback)(void* user, const soc_globals* g, const soc_frame_images* images, soc_stream stream);
/* Add a caller pass. before = name of the pass it precedes, or NULL to append at the end of its phase.
 * Caller passes survive soc_renderer_set_raster_scene. Errors: duplicate name, unknown `before` or a `before`
 * in another phase, bad resource id, more than SOC_PASS_MAX_USES uses. */
int soc_renderer_add_pass(soc_renderer* r, const soc_pass_desc* desc, soc_pass_callback fn, void* user,
                          const char* before);
/* Add the reference's ScreenSpaceReflection task (soc_screen_space_reflection) as a library-owned pass: name
 * "ScreenSpaceReflection", group "Screen Space Reflections", phase PRE, reads {ALBEDO, NORMAL, DEPTH,
 * metallic_roughness_resource}, writes {target_resource}; both resource ids in SOC_RES_USER0 .. SOC_RES_USER0 + 31 (the
 * metallic-roughness image and the ssr image are not frame images: the caller owns them and keeps them alive). `steps`
 * as in soc_screen_space_reflection (data NULL = none). before = NULL places it where the reference registers it
 * (renderer.cpp:1081-1092): before the pass whose name begins with "CloudRendering". pass_flags: 0, or SOC_PASS_ASYNC to
 * run it on the second lane. Like a caller pass it survives soc_renderer_set_raster_scene; errors as
 * soc_renderer_add_pass. Opt-in: a renderer that never calls this runs no SSR. */
int soc_renderer_add_screen_space_reflection(soc_renderer* r, soc_img metallic_roughness, soc_img target, soc_img steps,
                                             int32_t metallic_roughness_resource, int32_t target_resource,
                                             uint32_t pass_flags /* 0 or SOC_PASS_ASYNC */, const char* before);
/* Add the reference's depth-of-field tasks as two library-owned passes, both in group "Depth Of Field", phase PRE, on
 * the main lane: "MipMapping" (soc_depth_of_field_mips: the blit and every level; reads {COLOR}, writes
 * {chain_resource}) and, directly after it, "DepthOfField" (soc_depth_of_field; reads {chain_resource, DEPTH}, writes
 * {COLOR}). `chain`: the caller-owned RGBA16F chain of the frame's extent, kept alive; chain_resource in SOC_RES_USER0 ..
 * SOC_RES_USER0 + 31. before = NULL places the pair where the reference has them (renderer.cpp:1119-1153): directly
 * before "GenerateLuminanceHistogram". Requires a renderer created with SOC_RENDERER_UNFUSED_HISTOGRAM: the fused pass
 * bins the colour as Composition writes it, and the reference's histogram reads the blurred colour. Like caller passes
 * they survive soc_renderer_set_raster_scene; on any error the graph is left as it was (errors as
 * soc_renderer_add_pass). Opt-in: a renderer that never calls this runs no depth of field. */
int soc_renderer_add_depth_of_field(soc_renderer* r, soc_img chain, int32_t chain_resource, const char* before);
/* Declared uses of pass `index` as resource bitmasks (bit = enum soc_resource). */
int soc_renderer_pass_uses(const soc_renderer* r, int32_t index, uint64_t* reads, uint64_t* writes);
/* Derived dependencies of pass `index`: the indices of the earlier passes it must follow (ascending).
 * Returns their count (at most cap are written) or a negative error. */
int32_t soc_renderer_pass_dependencies(const soc_renderer* r, int32_t index, int32_t* out, int32_t cap);
/* Derived cross-frame (ring) dependencies of pass `index`: the passes of the PREVIOUS frame it must follow, for the
 * resources no earlier pass of its own frame writes (e.g. GBufferGeneration's depth write after the previous
 * frame's CloudRendering read it; CloudRendering's sky-colour write after the previous frame's TAA read the colour).
 * Indices ascending; returns their count (at most cap written) or a negative error. Cross-lane ring edges are
 * enforced by waits on the source pass's completion event; the fork at the start of a call orders the second lane
 * after everything queued on `stream` before the call. */
int32_t soc_renderer_pass_carry_dependencies(const soc_renderer* r, int32_t index, int32_t* out, int32_t cap);
/* Derived lane of pass `index` with the second lane enabled: 0 = the caller's stream, 1 = the second lane. */
int32_t soc_renderer_pass_lane(const soc_renderer* r, int32_t index);

/* --- Rasterisation: depth prepass, G-buffer and sun shadow map ---------------
 * Replaces the raster producers upstream of the hot path: DepthPrepassTask (depth_prepass.inl:26-120),
 * GBufferGenerationTask (g_buffer_generation.inl:33-230) and SunShadowDrawTask (sun_shadow_draw.inl:27-91).
 * A visibility buffer (one u64 per pixel: depth bits << 32 | triangle key) is filled by 64-bit atomicMin,
 * then one per-pixel resolve writes the reference's G-buffer images. Raster rules (the Vulkan ones the
 * reference pipelines select): pixel centres, a consistent tie rule for centres on shared edges (each is
 * covered once), depth clipping to [0, 1], LESS_OR_EQUAL test in draw order
 * (equal depth: the later triangle wins), culling by facing. Front faces are CLOCKWISE in the framebuffer
 * (Vulkan area a < 0): the reference culls FRONT for its glTF meshes, whose outward faces are counter-
 * clockwise as seen, so its pipelines' (Daxa default, not in the mount) front face must be clockwise.
 * Edge functions are homogeneous (2DH), so geometry behind the eye needs no clipping. A soc_mesh is
 * one mesh with one transform (the reference's draws concatenated); a scene of per-entity draws with their own
 * transforms is a soc_draw_scene ("Draw scenes" below). */
typedef struct soc_mesh {              /* device pointers (Vertex, shared.inl:152-157) */
    const float* positions;            /* vertex_count x float3, object space */
    const float* normals;              /* vertex_count x float3, object space */
    const float* uvs;                  /* vertex_count x float2 */
    const uint32_t* indices;           /* triangle_count x 3 */
    const uint32_t* materials;         /* triangle_count material indices, or NULL (all 0) */
    int32_t vertex_count, triangle_count;
    float model_matrix[16];            /* TransformComponent.model_matrix (column-major) */
    float normal_matrix[16];           /* TransformComponent.normal_matrix; its upper 3x3 transforms normals */
} soc_mesh;

/* Material (shared.inl:159-170, as GBufferGeneration's fragment shader reads it, g_buffer_generation.inl:
 * 189-225): albedo = sample(albedo).rgb * albedo_factor + emissive; emissive = sample(emissive).rgb *
 * emissive_factor (zero without an emissive image). Textures are RGBA8 (SRGB decoded to linear per
 * texel), bilinear, REPEAT; data == NULL samples white (model.cpp:188). Without SOC_MATERIAL_MIPMAPPED only
 * level 0 is read; with it every RGBA8 texture of the material carries its packed mip chain
 * (soc_generate_mips) and is sampled trilinear + anisotropic (the reference's sampler, texture.cpp:121-136):
 * see SOC_MATERIAL_MIPMAPPED. */
typedef struct soc_material {
    soc_img albedo, emissive;
    float albedo_factor[4], emissive_factor[4];
    int32_t flags;                     /* SOC_MATERIAL_* */
    int32_t has_emissive;              /* 0: emissive = 0 (has_emissive_image) */
    float alpha_cutoff;                /* with SOC_MATERIAL_ALPHA_MASK: the glTF alphaCutoff ("Alpha-masked materials") */
    int32_t pad;
    soc_img normal_map;                /* RGBA16F, used with SOC_MATERIAL_NORMAL_MAP */
    soc_img normal_image;              /* RGBA8_UNORM tangent-space normal texture, with SOC_MATERIAL_NORMAL_TEXTURE */
    float max_anisotropy;              /* with SOC_MATERIAL_MIPMAPPED: 16 in the reference (texture.cpp:129-130) */
    int32_t pad2;
    /* optional, read only with SOC_MATERIAL_PAIRED_TEXELS set (with SOC_MATERIAL_MIPMAPPED and a normal_image of the
     * albedo's extent): the two mip chains interleaved texel by texel (soc_pair_textures), which the G-buffer resolve
     * then reads with one load per texel row pair for both textures (the same texels and results); without the flag
     * the two images are read separately. The field took bytes that were padding before: zero-initialise the struct. */
    void* paired_texels;
} soc_material;
#define SOC_MATERIAL_ZERO_VELOCITY 1   /* write velocity 0 (the terrain draw, draw_terrain.inl:221) */
#define SOC_MATERIAL_NORMAL_MAP 2      /* normal = normalize(bilinear normal_map(uv).xyz) (draw_terrain.inl:206-219) */
/* has_normal_image (g_buffer_generation.inl:197-211): n = normalize(TBN * (sample(normal_image).xyz * 2 - 1)) with
 * T = normalize(Q1 * st2.t - Q2 * st1.t), B = normalize(cross(N, T)); Q1/Q2 and st1/st2 are dFdx/dFdy of the world
 * position and uv, taken as FINE derivatives: the same triangle's perspective-correct attributes at the two pixel
 * centres of the pixel's 2x2 quad in that direction (what helper invocations evaluate). */
#define SOC_MATERIAL_NORMAL_TEXTURE 4
/* Mip-mapped sampling (texture.cpp:108-136: LINEAR min/mag/mip, REPEAT, anisotropy max_anisotropy, lod in
 * [0, levels]). Per texture, from the FINE uv derivatives of the pixel's quad (as the TBN above), in level-0
 * texels: Px = |(du/dx W, dv/dx H)|, Py = |(du/dy W, dv/dy H)|, N = min(ceil(Pmax / Pmin), floor(max_anisotropy))
 * (1 when max_anisotropy <= 1, Pmax is 0 or not finite; floor(max_anisotropy) when Pmin is 0),
 * lod = log2(Pmax / N) (the deterministic log2 of the histogram contract) rounded to 1/256 and clamped to
 * [0, levels - 1]; result = (1/N) sum_{i=1..N} trilinear(uv + (i / (N + 1) - 1/2) d_major) with d_major the uv
 * derivative of the longer axis (EXT_texture_filter_anisotropic's reference filter; N = 1 samples uv itself);
 * trilinear = lerp of the bilinear REPEAT samples of levels floor(lod) and floor(lod) + 1. */
#define SOC_MATERIAL_MIPMAPPED 8
/* paired_texels holds the soc_pair_textures buffer of this material's albedo + normal_image (explicit opt-in: a caller
 * that fills the struct field by field without zeroing it never has stale padding read as a pointer) */
#define SOC_MATERIAL_PAIRED_TEXELS 16
/* glTF alphaMode MASK: a cutout material. Read ONLY by the *_masked raster calls ("Alpha-masked materials" below); every
 * other entry point, the resolve included, ignores it. */
#define SOC_MATERIAL_ALPHA_MASK 32

#define SOC_CULL_NONE 0
#define SOC_CULL_FRONT 1               /* depth prepass / G-buffer (depth_prepass.inl:45) */
#define SOC_CULL_BACK 2                /* sun shadow (sun_shadow_draw.inl:46) */

/* Workspace of the raster passes for a mesh (screen-space vertices, large-triangle list). */
size_t soc_raster_workspace_size(int32_t vertex_count, int32_t triangle_count);
/* Visibility buffer (u64 per pixel, width*height, tight): clear = 1 resets it to "empty, depth 1.0"
 * first. `view_projection` is the camera's projection*view (camera_projection_view_matrix). */
int soc_raster_visibility(const soc_mesh* mesh, const float view_projection[16], int32_t cull,
                          uint64_t* visibility, int32_t width, int32_t height, int32_t clear,
                          void* workspace, soc_stream stream);
/* Depth-only raster into a D32 image (cleared to 1.0), with the pipeline's depth bias: z += slope *
 * max(|dz/dx|, |dz/dy|) + constant * 2^(e - 23), e = the exponent of the triangle's largest |z|
 * (sun_shadow_draw.inl:47-50: 1.25 / 1.75). */
int soc_raster_depth(const soc_mesh* mesh, const float view_projection[16], int32_t cull, float bias_constant,
                     float bias_slope, soc_img depth, void* workspace, soc_stream stream);
/* G-buffer from a visibility buffer: depth (D32), albedo / emissive / normal / velocity (RGBA16F), with the
 * clear values of GBufferGeneration for empty pixels. `d_materials` is a device array. `workspace`
 * (soc_raster_workspace_size bytes, may be the raster's) lets the vertex stage run once per vertex;
 * NULL evaluates it per pixel. Same bits either way. */
int soc_gbuffer_resolve(const soc_globals* g, const soc_mesh* mesh, const soc_material* d_materials,
                        int32_t material_count, const uint64_t* visibility, soc_img depth, soc_img albedo,
                        soc_img emissive, soc_img normal, soc_img velocity, void* workspace, soc_stream stream);

/* DrawTerrain / SunShadowDrawTerrain patch tessellation (renderer.cpp:194-220 builds a grid_size^2 uv control
 * grid, 100 in the reference, of 4-point quad patches; draw_terrain.inl:144-191 tessellates each at
 * terrain_max_tess_level (3) with fractional_odd_spacing and displaces it by (heightmap(uv).r -
 * terrain_midpoint) * terrain_height_scale). Odd integer levels only (n equal segments). Output: the
 * ((grid - 1) n + 1)^2 shared vertices in world space (x = u scale.x - offset.x, y = offset.y + height,
 * z = v scale.y - offset.z; the TES's clip-space point before the linear clip transform), up normals (the
 * G-buffer normal comes from the terrain normal map), uvs, and 2 triangles per tessellated quad,
 * counter-clockwise seen from above. Heightmap: RGBA8_UNORM, bilinear clamp-to-edge (.r). */
int soc_terrain_tess_counts(int32_t grid_size, int32_t tess_level, int32_t* vertices, int32_t* triangles);
int soc_terrain_tessellate(const soc_globals* g, soc_img heightmap, int32_t grid_size, int32_t tess_level,
                           float* positions, float* normals, float* uvs, uint32_t* indices, soc_stream stream);

/* Texture mip chains (texture.cpp:108, 184-246): floor(log2(max(W, H))) + 1 levels, level k of max(1, W >> k) x
 * max(1, H >> k) texels. Packed chain layout: level 0 is the soc_img itself (any pitch); level k >= 1 follows at
 * data + pitch_bytes * H + sum_{1 <= j < k} 4 w_j h_j with tight rows. soc_mip_chain_bytes is the size of the
 * whole allocation (level 0 included). */
int32_t soc_mip_level_count(int32_t width, int32_t height);
size_t soc_mip_chain_bytes(int32_t width, int32_t height, int32_t pitch_bytes);
/* The load-time blit chain (texture.cpp:190-246): level k from level k-1 by a LINEAR blit (vkCmdBlitImage):
 * destination texel (x, y) samples the source at ((x + 0.5) Ws / Wd, (y + 0.5) Hs / Hd) bilinearly, clamp to
 * edge, 8-bit sub-texel weights; RGBA8_SRGB filters in linear space (per-texel decode, re-encoded to the
 * nearest sRGB code: the largest k with linear >= the midpoint of codes k-1 and k), RGBA8_UNORM and alpha
 * round to nearest. Runs once per texture at load (upload), one launch per level on `stream`. */
int soc_generate_mips(soc_img texture, soc_stream stream);
/* A material's albedo and normal image mip chains (both generated, one extent) interleaved texel by texel into
 * `paired` (soc_paired_texels_bytes(width, height) bytes, device): level k holds, for texel i of its tight
 * w_k x h_k rows, the albedo texel then the normal texel (8 B), levels packed after one another from level 0.
 * Runs once per material at load, on `stream`. */
size_t soc_paired_texels_bytes(int32_t width, int32_t height);
int soc_pair_textures(soc_img albedo, soc_img normal_image, void* paired, soc_stream stream);

/* HeightToNormalTask (height_to_normal.inl:52-83): RGBA8 heightmap (.r) -> RGBA16F normal map of the same
 * extent; run once at terrain load (renderer.cpp:158-190). */
int soc_height_to_normal(soc_img heightmap, soc_img normal_target, soc_stream stream);

/* GenerateMinHIZTask / GenerateMaxHIZTask (generate_min_hiz.inl:23-95, generate_hiz.glsl:17-98): single-pass
 * min (op_max = 0) or max depth pyramid. mips[i] is D32 of (W/2 >> i) x (H/2 >> i) (at least 1), i <
 * mip_count <= 12 (the reference uses ceil(log2(max(W, H) / 2)) levels); `counter` is one device u32 of
 * scratch (reset by the call). Computed but unused by the reference graph (quirk Q12). */
int soc_generate_hiz(const soc_globals* g, soc_img depth, const soc_img* mips, int32_t mip_count, int32_t op_max,
                     uint32_t* counter, soc_stream stream);

/* Render-graph raster head (renderer.cpp:965-1021: DepthPrepass, SunShadowDraw, GBufferGeneration): with a
 * scene set, every PRE phase first rasterises the mesh into the frame's G-buffer images (depth, albedo,
 * emissive, normal, velocity) and, with `shadow`, the sun shadow map into images.shadow, on the caller's
 * stream before the sky lane forks. The renderer copies the struct (the arrays stay caller-owned). Passes
 * are rebuilt: per-pass timing set before this call is re-enabled only through SOC_RENDERER_TIMING. */
typedef struct soc_raster_scene {
    soc_mesh mesh;                     /* device arrays */
    const soc_material* materials;     /* device array */
    int32_t material_count;
    int32_t shadow;                    /* 1: SunShadowDraw into images.shadow (cull BACK, bias 1.25 / 1.75) */
    uint64_t* visibility;              /* width*height u64, device */
    void* workspace;                   /* soc_raster_workspace_size(mesh) bytes, device */
} soc_raster_scene;
/* NULL: clear. With shadow = 1 the renderer allocates a second raster workspace (soc_raster_workspace_size of the mesh)
 * for the sun shadow draw, which then runs on its second lane beside the depth prepass and the G-buffer. */
int soc_renderer_set_raster_scene(soc_renderer* r, const soc_raster_scene* scene);

/* --- Draw scenes: per-entity draws with their own transforms ------------------------------------
 * The reference draws a scene of entities: GBufferGenerationTask (g_buffer_generation.inl:111-144), DepthPrepassTask
 * (depth_prepass.inl) and SunShadowDrawTask (sun_shadow_draw.inl) walk scene->iterate, bind every mesh entity's
 * TransformComponent buffer (model_matrix, normal_matrix) and issue one draw_indexed {index_count, first_index,
 * vertex_offset} per primitive with the primitive's material in the push constant. A draw scene is that loop as
 * data: shared vertex arrays, one index array, a host array of draws and a device array of transforms. Results are
 * those of the serial draw loop: the global triangle id of draw d's local triangle t is sum(triangle_count of the
 * draws before d) + t; the visibility key stays depth bits << 32 | (0xFFFFFFFE - id), so at equal depth the later
 * draw, and within a draw the later triangle, wins (LESS_OR_EQUAL in draw order). Every vertex of a draw goes through
 * the single-mesh vertex arithmetic with that draw's matrices (the same bits as a soc_mesh holding the draw). Culling,
 * depth clipping, bias and clear values are unchanged. Velocity follows the reference: the previous clip position uses
 * the CURRENT model matrix (g_buffer_generation.inl:171); per-object motion vectors from the previous frame's
 * transforms are opt-in ("Draw scenes: per-object motion vectors" below). */
typedef struct soc_transform {         /* TransformComponent buffer; what soc_scene_update writes per entity */
    float model_matrix[16];            /* column-major */
    float normal_matrix[16];           /* its upper 3x3 transforms normals */
} soc_transform;
typedef struct soc_draw {              /* one draw_indexed of one entity (g_buffer_generation.inl:135-143) */
    int32_t first_index;               /* first element of the index array */
    int32_t triangle_count;            /* index_count / 3 of the primitive (0: an empty draw) */
    int32_t vertex_offset;             /* signed, added to every fetched index */
    int32_t first_vertex, vertex_count;/* the vertex range the draw's offset indices must fall in */
    int32_t transform;                 /* index into the transform array */
    int32_t material;                  /* primitive.material_index: one material for every triangle of the draw */
} soc_draw;
/* Non-indexed primitives are expressed with an identity index range. Several draws may name one vertex range with
 * different transforms (two entities, one Model): each gets its own transformed copy of the range per frame. */
typedef struct soc_draw_scene {
    const float* positions;            /* device, vertex_count x float3, object space */
    const float* normals;              /* device, vertex_count x float3 (the G-buffer resolve needs it) */
    const float* uvs;                  /* device, vertex_count x float2 (the G-buffer resolve needs it) */
    const uint32_t* indices;           /* device, index_count entries */
    int32_t vertex_count, index_count;
    const soc_draw* draws;             /* HOST array, draw order */
    int32_t draw_count;
    int32_t transform_count;
    const soc_transform* transforms;   /* device; rewritten by the caller between frames (no rebuild needed) */
    int32_t material_count;            /* every draw's material is below it */
    int32_t pad;
    void* workspace;                   /* device, soc_draw_workspace_size(draws, draw_count) bytes, 256-byte aligned */
} soc_draw_scene;
/* Workspace of a draw list (pure host; 0 on bad input: null draws, a negative count or field, more than 2^31 - 1
 * triangles or transformed vertices in all). Layout: the static tables built by
 * soc_draw_scene_build (per transformed-vertex slot its source vertex, transform and uv; the index buffer rebased to
 * the slots in global triangle order; the per-triangle material), then one single-mesh raster workspace
 * (soc_raster_workspace_size of the slot and triangle totals) per view: the camera's (soc_raster_visibility_draws,
 * soc_gbuffer_resolve_draws) and the sun's (soc_raster_depth_draws), so the two may run on different streams. There
 * is one slot per (draw, vertex of its range). */
size_t soc_draw_workspace_size(const soc_draw* draws, int32_t draw_count);
/* Load-time build of the static tables, run once and again whenever the draws, the indices or the uvs change (not
 * when the transforms do). Everything the host can check is checked before the first HIP call (SOC_E_INVALID_ARG:
 * null pointers, bad counts; SOC_E_SHAPE: first_index + 3 triangle_count > index_count, a vertex range outside
 * vertex_count, transform >= transform_count, material >= material_count, 0xFFFFFFFE triangles or more). The build
 * then validates ON THE DEVICE that every fetched index + vertex_offset lies in the draw's [first_vertex, first_vertex
 * + vertex_count) before any kernel addresses a vertex with it, synchronises `stream` to read the result back and
 * returns SOC_E_SHAPE with the first offending draw in soc_last_error_string(). The library remembers the outcome per
 * workspace: the *_draws entry points refuse (without a launch) a scene that was not built, whose description changed
 * since, or whose build failed. Call soc_draw_scene_release before freeing or reusing the workspace. */
int soc_draw_scene_build(const soc_draw_scene* scene, soc_stream stream);
/* Forgets what the library remembers of the scene's workspace (NULL or an unknown workspace: no-op). */
void soc_draw_scene_release(const soc_draw_scene* scene);
/* The single-mesh entry points' twins, with the scene in place of the mesh (same arguments otherwise, no workspace:
 * the scene carries it). The draw-aware vertex kernels run per call with the transforms as they are on `stream`;
 * the triangle and pixel kernels are the single-mesh ones, on the rebased tables. soc_raster_visibility_draws and
 * soc_gbuffer_resolve_draws share the camera view's buffers (order them on one stream, resolve after visibility);
 * soc_raster_depth_draws uses the sun view's. The resolve always uses the per-vertex workspace. */
int soc_raster_visibility_draws(const soc_draw_scene* scene, const float view_projection[16], int32_t cull,
                                uint64_t* visibility, int32_t width, int32_t height, int32_t clear, soc_stream stream);
int soc_raster_depth_draws(const soc_draw_scene* scene, const float view_projection[16], int32_t cull,
                           float bias_constant, float bias_slope, soc_img depth, soc_stream stream);
int soc_gbuffer_resolve_draws(const soc_globals* g, const soc_draw_scene* scene, const soc_material* d_materials,
                              int32_t material_count, const uint64_t* visibility, soc_img depth, soc_img albedo,
                              soc_img emissive, soc_img normal, soc_img velocity, soc_stream stream);
/* The raster head from a draw scene: DepthPrepass, SunShadowDraw (with `shadow`), GBufferGeneration, with the names,
 * groups, declared uses and lanes soc_renderer_set_raster_scene gives. Replaces a scene set by
 * soc_renderer_set_raster_scene and the other way round; NULL clears. The renderer copies the struct and the draw
 * array; the device arrays stay caller-owned. It keeps the device pointer to the transforms: the caller rewrites that
 * array on its own stream between frames and the next soc_renderer_execute sees it, like every frame input (written
 * on the caller's stream before the call). The sun shadow draw reads it on the second lane behind the call's fork,
 * also under SOC_RENDERER_STATIC_INPUTS (see there). */
int soc_renderer_set_draw_scene(soc_renderer* r, const soc_draw_scene* scene, const soc_material* d_materials,
                                int32_t material_count, int32_t shadow, uint64_t* visibility);

/* --- Alpha-masked materials: cutout coverage (opt-in) --------------------------
 * The reference has no alpha test (no `discard` in its shaders): a glTF alphaMode MASK material renders as solid
 * geometry there and in every call above. The four *_masked calls are the raster calls' twins with a material table
 * (device array, as the resolve takes it): a fragment of a triangle whose material has SOC_MATERIAL_ALPHA_MASK is kept
 * or discarded by the test below after the coverage rules have accepted the pixel; a discarded fragment writes
 * nothing (neither a key nor a depth). Triangles of other materials take the unmasked path, and a table without a
 * flagged material gives the bits of the unmasked twin. The material of triangle t is
 * min(mesh.materials[t], material_count - 1), 0 when mesh.materials is NULL (the resolve's clamp); for a draw scene
 * the draw's material. All arithmetic is fp32, each operation rounded on its own (no contraction):
 *   1. es = e0 + e1 + e2; b1 = e1 / es; b2 = e2 / es; b0 = 1 - b1 - b2, with e_i the raster's three edge values at the
 *      pixel centre (the resolve's barycentrics, bit for bit);
 *   2. u = b0 uvA.x + b1 uvB.x + b2 uvC.x, v likewise (the resolve's expression, in its order; a draw scene: the uvs of
 *      the triangle's transformed-vertex slots);
 *   3. LEVEL 0 of `albedo`, always, also under SOC_MATERIAL_MIPMAPPED and SOC_MATERIAL_PAIRED_TEXELS: REPEAT on each
 *      axis with the sampling contract's 8-bit weights kx, ky (any extent, the image's pitch), the four texels' alpha
 *      bytes, A = (a00 (256 - kx) + a10 kx) (256 - ky) + (a01 (256 - kx) + a11 kx) ky, an integer <= 255 * 65536;
 *   4. alpha = (float)A * (1.0f / (255.0f * 65536.0f));
 *   5. kept iff alpha * albedo_factor[3] >= alpha_cutoff. A NaN on either side discards. albedo.data == NULL: alpha 1.
 * Level 0 is deliberate: uv derivatives do not exist before visibility is resolved, and level 0 keeps thin cutouts
 * (a chain, a fence) from eroding with distance, which the averaged alpha of the lower levels does. The decision is
 * exact by specification: results are compared bit for bit, without a tolerance. A visible fragment's G-buffer values
 * do not depend on the test, so soc_gbuffer_resolve(_draws) reads a masked visibility buffer as it reads any other.
 * alphaMode BLEND has no place in a deferred frame (one surface per pixel) and is rendered opaque.
 * Errors, all before the first HIP call: the twin's, and SOC_E_INVALID_ARG for null d_materials, material_count <= 0,
 * null uvs (mesh or scene), or (draw scenes) material_count < scene->material_count. Workspaces are the twins'. */
int soc_raster_visibility_masked(const soc_mesh* mesh, const float view_projection[16], int32_t cull,
                                 uint64_t* visibility, int32_t width, int32_t height, int32_t clear, void* workspace,
                                 const soc_material* d_materials, int32_t material_count, soc_stream stream);
int soc_raster_depth_masked(const soc_mesh* mesh, const float view_projection[16], int32_t cull, float bias_constant,
                            float bias_slope, soc_img depth, void* workspace, const soc_material* d_materials,
                            int32_t material_count, soc_stream stream);
int soc_raster_visibility_draws_masked(const soc_draw_scene* scene, const float view_projection[16], int32_t cull,
                                       uint64_t* visibility, int32_t width, int32_t height, int32_t clear,
                                       const soc_material* d_materials, int32_t material_count, soc_stream stream);
int soc_raster_depth_draws_masked(const soc_draw_scene* scene, const float view_projection[16], int32_t cull,
                                  float bias_constant, float bias_slope, soc_img depth, const soc_material* d_materials,
                                  int32_t material_count, soc_stream stream);
/* Render graph: with enable != 0 and a raster head set (mesh or draw scene), DepthPrepass and SunShadowDraw (every
 * cascade slab included) call the masked twins with the head's own material table. A renderer flag: no HIP call, no
 * pass is rebuilt; names, groups, lanes and declared uses stay, and the flag survives a change of head. The terrain
 * layer's passes stay unmasked (the reference's terrain material is opaque; DrawTerrain depth-tests against the depth
 * image and so sees the cutouts). SOC_E_INVALID_ARG: null renderer. */
int soc_renderer_set_alpha_mask(soc_renderer* r, int32_t enable);

/* --- Draw scenes: per-object motion vectors (opt-in) ----------------------------
 * The reference forms the previous clip position with the CURRENT model matrix, so the velocity of an entity that moved
 * holds the camera's motion only and TAA reprojects it from where it never was. soc_gbuffer_resolve_draws_motion is
 * soc_gbuffer_resolve_draws with one more device array, the transforms of the PREVIOUS frame (same index, same
 * transform_count entries as scene->transforms; only each model_matrix is read): the previous clip position of a vertex
 * of draw d becomes previous_vp . (previous[d.transform].model_matrix . p), the current-frame chain's operations in its
 * order. Everything else (depth, albedo, emissive, normal, the current clip position) is computed as before. A draw
 * whose previous model matrix equals its current one bit for bit gets the bits of soc_gbuffer_resolve_draws, and
 * previous_transforms == scene->transforms (the arrays may alias) reproduces that call entirely. The same host-side
 * checks and refusals of an unbuilt, changed or failed workspace, all before any HIP call; a NULL previous_transforms
 * is SOC_E_INVALID_ARG. */
int soc_gbuffer_resolve_draws_motion(const soc_globals* g, const soc_draw_scene* scene,
                                     const soc_transform* previous_transforms, const soc_material* d_materials,
                                     int32_t material_count, const uint64_t* visibility, soc_img depth, soc_img albedo,
                                     soc_img emissive, soc_img normal, soc_img velocity, soc_stream stream);
/* The render graph's GBufferGeneration with per-object motion. `previous_transforms` is CALLER memory like the
 * transforms (device, the draw scene's transform_count entries) that the RENDERER writes: GBufferGeneration calls the
 * motion resolve with it and then copies the current transforms into it for the next frame, on the caller's stream
 * inside the same pass (after the resolve's vertex stage, so before the caller's next rewrite of the transforms by
 * stream order; nothing is allocated, no pass is added: names, groups, declared uses and lanes stay as they are). The
 * first frame after this call copies current -> previous before the vertex stage too, so it gives the reference's
 * velocity. NULL turns motion off. SOC_E_INVALID_ARG when no draw scene is set. soc_renderer_set_draw_scene and
 * soc_renderer_set_raster_scene (with a scene or NULL) turn motion off again: a new scene may have another transform
 * count. The history array is not renderer state: it is not part of the Python Renderer's save_state / load_state. A
 * caller who wants continuity after load_state restores the array's contents itself (the transforms of the frame
 * before the checkpoint) in a renderer whose motion is on and has run a frame; this call itself always restarts the
 * history, so the frame after it has the reference's velocity. */
int soc_renderer_set_draw_motion(soc_renderer* r, soc_transform* previous_transforms);

/* --- Terrain layer: DrawTerrain / SunShadowDrawTerrain over the raster head (opt-in) ----------
 * The reference's frame is entities standing on terrain: rebuild_task_graph (renderer.cpp:965-1021) runs DepthPrepass,
 * SunShadowDraw, SunShadowDrawTerrain, GBufferGeneration and DrawTerrain, and both terrain tasks LOAD the images the
 * entity tasks wrote and depth-test into them with LESS_OR_EQUAL. The two calls below are those tasks for any soc_mesh
 * (soc_terrain_tessellate's, or any other).
 *
 * soc_draw_terrain. The mesh is rasterised into `visibility` (width*height u64 of `depth`'s extent, cleared by the
 * call; cull FRONT, the rules and the key of soc_raster_visibility with the globals' camera_projection_view_matrix). A
 * pixel with a terrain fragment of depth z_t reads the depth image's value z_e; the fragment wins iff z_t <= z_e,
 * compared on the float bits the key carries (exact; both depths are >= +0, as every depth this library writes), so a
 * tie goes to the terrain, the later draw. A winning pixel writes depth = z_t and albedo, normal and velocity as
 * soc_gbuffer_resolve computes them for that triangle and material (the reference's terrain material is
 * SOC_MATERIAL_ZERO_VELOCITY | SOC_MATERIAL_NORMAL_MAP: velocity (0, 0, 0, 0), draw_terrain.inl:220). There is NO
 * emissive image: DrawTerrain has three colour attachments (draw_terrain.inl:14-17, 199-201), so where the terrain hides
 * an entity the emissive image keeps the hidden entity's value, and bloom and composition see it. A losing or empty
 * pixel writes nothing at all. `workspace` (soc_raster_workspace_size of the mesh) is required: the layer always runs
 * the vertex stage once per vertex.
 *
 * soc_sun_shadow_draw_terrain. Depth-only raster of the mesh into the D32 shadow image, cull BACK and NO depth bias
 * (sun_shadow_draw_terrain.inl:47-58 has no depth_bias_*), with clear = 0 on top of what is there (the image
 * SunShadowDraw left): the 32-bit atomicMin gives the per-texel minimum of the two whatever the order. clear = 1 clears
 * to 1.0 first, for a frame whose head draws no shadow; it then equals soc_raster_depth with bias 0 / 0.
 * Quirk Q15: the reference's shadow terrain ignores terrain_offset (its vertex is (u sx, 0 + height, v sz),
 * sun_shadow_draw_terrain.inl:112, against draw_terrain.inl:141), so with a non-zero offset its shadow is not under
 * its terrain. Both calls take a mesh, so a caller who wants the quirk tessellates a second mesh with a globals copy
 * whose terrain_offset is zero (x - 0.0f is exact) and passes that one here; the default offset is zero and one mesh
 * serves both.
 *
 * Every refusal is made on the host before the first HIP call, with soc_last_error_string() set: a null mesh,
 * visibility or workspace and check failures of the mesh (SOC_E_INVALID_ARG; SOC_E_SHAPE for too many triangles),
 * material_count <= 0, images of wrong formats (SOC_E_INVALID_ARG) or differing extents (SOC_E_SHAPE). */
int soc_draw_terrain(const soc_globals* g, const soc_mesh* mesh, const soc_material* d_materials,
                     int32_t material_count, uint64_t* visibility /* W*H, cleared by the call */,
                     soc_img depth, soc_img albedo, soc_img normal, soc_img velocity,
                     void* workspace, soc_stream stream);
int soc_sun_shadow_draw_terrain(const soc_mesh* mesh, const float view_projection[16], int32_t clear,
                                soc_img depth, void* workspace, soc_stream stream);
typedef struct soc_terrain_layer {
    soc_mesh mesh;                  /* camera view; device arrays (soc_terrain_tessellate, or any mesh) */
    soc_mesh shadow_mesh;           /* positions == NULL: use `mesh` */
    const soc_material* materials;  /* device */
    int32_t material_count, shadow;
    uint64_t* visibility;           /* may be the head's own buffer */
    void* workspace;                /* soc_raster_workspace_size(mesh) */
    void* shadow_workspace;         /* of the shadow mesh; required with shadow = 1 */
} soc_terrain_layer;
/* The render graph's terrain layer over a raster head (a mesh or a draw scene; SOC_E_INVALID_ARG without one). Adds
 * "DrawTerrain" directly after "GBufferGeneration" (group "Rendering G-Buffer", reads and writes VISIBILITY, DEPTH,
 * ALBEDO, NORMAL, VELOCITY, on the caller's stream; it writes the velocity image GBufferGeneration writes) and, with
 * `shadow`, "SunShadowDrawTerrain" (group "Shadows", reads and writes SUN_SHADOW) directly after "SunShadowDraw" on
 * that pass's lane with clear = 0, or, when the head draws no shadow, after "DepthPrepass" on the caller's stream with
 * clear = 1. Dependencies and ring edges are derived from the declared uses as for every pass. The renderer copies the
 * struct (the arrays stay caller-owned). The layer survives replacing the head by another head; it is removed with the
 * head (soc_renderer_set_raster_scene / _set_draw_scene with NULL) and by a NULL layer. Per-object motion is
 * unaffected. The layer's visibility buffer may be the head's (GBufferGeneration has read it by then); its workspaces
 * are its own. SOC_E_INVALID_ARG for an incomplete layer, shadow = 1 without a shadow_workspace or without
 * images.shadow. Passes are rebuilt as by soc_renderer_set_raster_scene. */
int soc_renderer_set_terrain(soc_renderer* r, const soc_terrain_layer* layer);   /* NULL removes it */

/* --- Headless output and metrics (replaces the swapchain present of tone_mapping.inl:
 * 172-176 and the ImGui "GPU Metric" window of renderer.cpp:769-806) ------------------------------- */
/* The most recent frame's timed passes as one JSON object: {"frame", "total_gpu_ms", "groups" (the 12
 * group names of renderer.cpp:577-588, 0 when absent), "passes"}. Writes at most cap-1 bytes + NUL;
 * returns the full length (snprintf-style) or < 0. Needs a completed stream. */
int64_t soc_renderer_metrics_json(soc_renderer* r, uint64_t frame, char* buf, size_t cap);
/* Device image -> host rows, stream-ordered. */
int soc_read_image(soc_img image, void* host, int32_t host_pitch_bytes, soc_stream stream);
/* 8-bit RGBA host image -> PNG file (uncompressed deflate; no external library). */
int soc_write_png(const char* path, const void* rgba8, int32_t width, int32_t height, int32_t pitch_bytes);
/* RGBA16F host image (e.g. the HDR composition / TAA colour) -> OpenEXR 2 scanline file, uncompressed HALF
 * channels (the f16 framebuffer dump; the reference reads EXR through tinyexr, texture.cpp:300-412). */
int soc_write_exr(const char* path, const void* rgba16f, int32_t width, int32_t height, int32_t pitch_bytes);

#ifdef __cplusplus
}
#endif

#endif /* SOC_RT_H */
