/*
 * rainhip.h -- C ABI of librainhip.so: the MI355X (gfx950) implementation of the
 * per-image rain-streak rendering + compositing hot path of
 * astra-vision/rain-rendering.
 *
 * The reference is pure Python and has no FFI; the boundary this library plugs
 * into is the per-frame body of Generator.run (reference common/generator.py:389-467)
 * and its two inner seams
 *     Generator.compute_drop              reference common/generator.py:119-191
 *     RainRenderer.add_drop_to_image      reference common/bad_weather.py:336-462
 * A maintainer binds it with ctypes.  Plain pointers and
 * sizes only; the caller owns every buffer; no function throws; every function
 * returns 0 or a negative RR_E* code and rr_last_error() explains it.
 *
 * There is NO CPU implementation behind this ABI: rr_create fails with
 * RR_E_NO_DEVICE when no gfx950 device is visible.
 */
#ifndef RAINHIP_H
#define RAINHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_VERSION 400            /* 0.4.0: + rr_frame_in.in_types (float32 / uint8 image and map inputs), float32 colour branch by default */

enum {
  RR_OK = 0,
  RR_E_ARG = -1,                  /* bad argument (null pointer, bad size, mixed frame sizes) */
  RR_E_NO_DEVICE = -2,            /* no HIP device / not gfx950 */
  RR_E_HIP = -3,                  /* a HIP runtime call failed */
  RR_E_STATE = -4,                /* streak DB or camera not set */
  RR_E_ARENA = -5,                /* tile arena overflow: arena regrown, enqueue / submit the batch again */
  RR_E_PARSE = -6,                /* rr_host_parse_particles: malformed file or missing / non-numeric attribute */
  RR_E_UNSUPPORTED = -7           /* rr_host_parse_particles: XML construct outside the simulator's subset (DOCTYPE, CDATA,
                                   * entity references): use a full XML parser */
};

/* per-drop status written to rr_frame_out.drop_status: 0 == composited.  The
 * reference expresses all of these as "exception inside add_drop_to_image ->
 * drop not composited" (common/generator.py:180-189). */
enum {
  RR_DROP_OK = 0,
  RR_DROP_FOV_FAIL = 1,           /* compute_fov_plane_points returned [] (bad_weather.py:698-704): e.g. > radius */
  RR_DROP_EMPTY_FOV = 2,          /* FOV polygon does not touch the envmap (bad_weather.py:372 IndexError) */
  RR_DROP_BAD_COC = 3,            /* non-finite circle of confusion (int(10*c) raises, bad_weather.py:293) */
  RR_DROP_TOO_BIG = 4             /* defocus pad > RR_MAX_SHIFT px: documented limit of this library */
};

#define RR_MAX_SHIFT 1024
#define RR_MAX_FOV 32

typedef struct rr_ctx rr_ctx;

struct rr_sim_frame;

/* Camera / renderer constants.  Mirrors RainRenderer(focal, f_number, focus_plane=6,
 * radius=10, fov=165) (generator.py:267), N=20 (generator.py:179) and the constants of
 * bad_weather.py:344-345,425,469.  Transcendental-derived values are computed ONCE by
 * the host with numpy so that device results do not depend on a device libm. */
typedef struct {
  double focal_m;                 /* settings["cam_focal"] / 1000 */
  double focal_sq;                /* focal_m ** 2 evaluated by the host (bad_weather.py:468) */
  double f_number;
  double focus_plane;             /* 6 */
  double exposure_s;              /* settings["cam_exposure"] / 1000 (bad_weather.py:344) */
  double radius;                  /* 10 */
  double sensor_px;               /* 4.65e-06 (bad_weather.py:469) */
  double tau_zero;                /* sqrt(1.16e-3) / 50 (bad_weather.py:425) */
  double fov_cos, fov_sin;        /* cos/sin(-deg2rad(fov/2)) (bad_weather.py:602,625) */
  double phi_cos[RR_MAX_FOV];     /* cos(k * 2*pi/N)  (bad_weather.py:630-634) */
  double phi_sin[RR_MAX_FOV];
  int32_t n_fov;                  /* 20 */
  int32_t reserved;
} rr_camera;

/* One streak that passed the frame filter (generator.py:413-420), as plain data.
 * The legacy-RandomState draws (bad_weather.py:252-264, generator.py:136) stay in
 * Python; their results arrive here as tex_index and rot_cos/rot_sin. */
typedef struct {
  int32_t x0, y0, x1, y1;         /* image_position_start / _end (ints, after the in-place noise rotation generator.py:152-161) */
  int32_t max_width;              /* Streak.max_width */
  int32_t length;                 /* Streak.length */
  int32_t type;                   /* DropType: 0 Big, 1 Medium, 2 Small */
  int32_t tex_index;              /* index into the streak DB chosen by take_drop_texture */
  double iw1, iw2;                /* image_diameter_start / _end */
  double wps[3], wpe[3];          /* world_position_start / _end (z already negated, bad_weather.py:223-224) */
  double rot_cos, rot_sin;        /* cos/sin(-(theta+noise) * pi/180) for imutils.rotate_bound (non-Big) */
} rr_drop;                        /* 112 bytes */

/* A caller-made tile for one drop: the seam of RainRenderer.add_drop_to_image (common/bad_weather.py:336-338), whose
 * arguments `drop` (the RGBA tile Generator.compute_drop built: gray, alpha == channel 0), `drop_minC` and `drop_fov_pts`
 * these are.  With alpha != NULL the library neither synthesises the streak tile nor evaluates the field-of-view polygon
 * of that drop; everything after that (colour, defocus, placement, blend) is the common path. */
typedef struct {
  const double* alpha;            /* th*tw values in [0,1], row-major; NULL: this drop is rendered the normal way */
  int32_t tw, th;
  int32_t min_x, min_y;           /* drop_minC */
  int32_t n_poly, reserved;       /* vertices of drop_fov_pts (<= RR_MAX_FOV + 4); 0: compute_fov_plane_points failed ([]) */
  const double* poly_xy;          /* n_poly (x, y) pairs, float pixels of the environment map (truncated like pyclipper does) */
} rr_ext_tile;

typedef struct {
  int32_t H, W;                   /* frame */
  int32_t He, We;                 /* lat-long environment map */
  /* the four arrays below are float64 unless in_types says otherwise */
  const void* bg;                 /* H*W*3 BGR, un-fogged image / 255 (used for the mean shift, generator.py:462) */
  const void* rainy_bg;           /* H*W*3 BGR, output of the fog pre-pass (generator.py:386): values in [0, 1] (it ends with
                                   * np.clip); a NaN stays a NaN like in the reference */
  const void* env_xyY;            /* He*We*3 (generator.py:407-408) */
  const void* omega;              /* He*We solid angles (generator.py:410); NULL: the map given to rr_set_solid_angles */
  const rr_drop* drops;           /* n_drops records in reference order */
  int32_t n_drops;
  int32_t strategy;               /* 0: default (rendering_strategy=None); 1: 'white' (bad_weather.py:349-353) */
  double opacity_attenuation;     /* --opacity_attenuation */
  const void* depth;              /* optional, only read with RR_OPT_DEPTH_OCCLUSION: scene depth in metres, H*W float32
                                   * (depth_f64 == 0) or float64; rr_pipeline_* use the pre-pass' depth instead */
  int32_t depth_f64;
  /* Element types of the image and map inputs (0: everything float64, the reference's arrays).  The three colour channels
   * and the drop colour only have to land within 1 LSB of a uint8 (BASELINE.json) and the mask never reads these arrays, so
   * a caller that holds them narrower hands them over as they are -- a third to an eighth of the HBM bytes:
   *   RR_IN_BG_F32 / RR_IN_BG_U8         `bg` is float32 / uint8 (uint8: the bytes cv2.imread returned; bg = bytes / 255.0)
   *   RR_IN_RAINY_F32 / RR_IN_RAINY_U8   the same for `rainy_bg` (when rainy_bg == bg the BG flags count for both)
   *   RR_IN_ENV_F32                      `env_xyY` AND `omega` (when not NULL) are float32; for every frame of a batch or for none
   * rr_render_frames_device and rr_render_frames; rr_pipeline_* produce rainy_bg / env_xyY themselves. */
  int32_t in_types;
  const rr_ext_tile* ext;         /* optional: n_drops entries (rr_render_frames / rr_render_frames_device only) */
  /* Drop tables born on the device (rr_generate_drops_device): with n_drops_dev != NULL (a DEVICE pointer to one int32;
   * rr_render_frames_device only) the frame's drop count is read from there when the kernels run, clamped to n_drops, which
   * then is the CAPACITY of `drops` (and of drop_status / drop_colour) the launch is sized for. */
  const int32_t* n_drops_dev;
  /* In-kernel particle simulation (BASELINE config 5; host-pointer entry points rr_render_frames / rr_pipeline_*): with
   * sim != NULL (HOST pointer to this frame's generator settings) the frame's drop table is generated on the device
   * (rr_generate_drops_device semantics) instead of uploaded: `drops` is ignored (may be NULL) and n_drops is the capacity
   * the launch is sized for (0: sim->n_particles).  The count comes back in rr_frame_out.n_drops_out. */
  const struct rr_sim_frame* sim;
} rr_frame_in;

enum { RR_IN_BG_F32 = 1, RR_IN_BG_U8 = 2, RR_IN_ENV_F32 = 4, RR_IN_RAINY_F32 = 8, RR_IN_RAINY_U8 = 16, RR_IN_BG_PNG_ROWS = 32, RR_IN_BG_JPEG = 64 };

typedef struct {
  uint8_t* rainy_rgb;             /* H*W*3 RGB: what plt.imsave(rainy_image) stores (generator.py:461-466), alpha omitted */
  double* rainy_bg_out;           /* optional (may be NULL): H*W*3 BGR composite before the mean shift */
  double* mask_f64;               /* H*W: rainy_mask accumulator (bad_weather.py:450); may be NULL */
  int32_t* mask_i32;              /* H*W: floor(mask_f64 * 255)  (SURVEY decision D1); may be NULL */
  int32_t* drop_status;           /* n_drops RR_DROP_* codes (may be NULL) */
  /* Optional: the two PNG files the reference writes per frame (generator.py:466-467), as PNG
   * scanlines ready for deflate: H rows of 1 + 4*W bytes = filter byte 1 (Sub) + the Sub-filtered RGBA pixels.
   * rainy_png: plt.imsave(rainy_image) (alpha 255); mask_png: plt.imsave(rainy_mask) = (mask - min) / (max - min) through
   * the 256-entry colour map given to rr_set_colormap (needs mask_f64 in the device-pointer entry points).
   * With RR_OPT_PNG_DEFLATE the same buffers come back entropy-coded (see the option): 16-byte header + the file's zlib stream. */
  uint8_t* rainy_png;
  uint8_t* mask_png;
  /* Optional: n_drops * 3 doubles, the B, G, R colour constants K of every drop: the tile colour the reference derives
   * from the environment map inside the drop's field of view (bad_weather.py:397-412) is K * gray value.  Zeros for a
   * drop that is not composited.  Lets the single-drop seam hand back the reference's `drop_vis` (bad_weather.py:462). */
  double* drop_colour;
  int32_t* n_drops_out;           /* optional: one int32, the number of drops of a generated drop table (rr_frame_in.sim) */
} rr_frame_out;

typedef struct {
  char name[32];
  int32_t launches;
  int32_t reserved;
  double total_ms;                /* sum of HIP-event durations */
} rr_kernel_stat;

int rr_version(void);

/* device: HIP ordinal.  Fails (RR_E_NO_DEVICE) without a gfx9 device. */
int rr_create(rr_ctx** out, int device);
int rr_destroy(rr_ctx* ctx);
const char* rr_last_error(rr_ctx* ctx);

/* SURVEY 8b's collective, for a host that drives several GPUs from ONE process: the streak database of ctxs[0]
 * (rr_set_streak_db / rr_set_streak_db_device) becomes the database of ctxs[1 .. n_ctx - 1] without a trip through the host.
 * Contexts on the root's device take a device-to-device copy; contexts on other devices an ncclBroadcast (RCCL over xGMI; one
 * communicator rank per device, librccl.so.1 loaded on first use -- RR_E_STATE if it cannot be).  Synchronous; the error text
 * is ctxs[0]'s rr_last_error.  n_ctx = 1 is a no-op.  (This repo's drivers run one PROCESS per GPU and broadcast through
 * torch.distributed -- sharding.py; the reference has no counterpart: main_threaded.py starts a process per sequence.) */
int rr_bcast_streak_db(rr_ctx** ctxs, int32_t n_ctx);
/* Diagnostic: the RCCL leg of rr_bcast_streak_db on the context's OWN device (a communicator of one rank; the database
 * broadcast into a scratch buffer and compared) -- what a box with one GPU can check of it. */
int rr_bcast_selftest(rr_ctx* ctx);

/* Streak database: n_tex gray uint8 textures, already normalised as
 * uint8((255*norm*img)/65535) (bad_weather.py:141), concatenated in `texels`
 * (host pointer) with per-texture height/width/offset. */
int rr_set_streak_db(rr_ctx* ctx, const uint8_t* texels, const int32_t* tex_h, const int32_t* tex_w,
                     const int64_t* tex_off, int32_t n_tex);
/* Same, but `texels` is a DEVICE pointer on ctx's device (e.g. the buffer that just
 * received the RCCL broadcast of the packed database). */
int rr_set_streak_db_device(rr_ctx* ctx, const uint8_t* texels_dev, int64_t n_bytes, const int32_t* tex_h,
                            const int32_t* tex_w, const int64_t* tex_off, int32_t n_tex);
int rr_set_camera(rr_ctx* ctx, const rr_camera* cam);
/* The solid-angle map of He x We environment maps (generator.py:410: a function of the map's shape alone), kept resident
 * on the device: frames of that map size may then pass omega == NULL instead of uploading it with every batch. */
int rr_set_solid_angles(rr_ctx* ctx, int32_t He, int32_t We, const double* omega);
/* 256 RGBA byte entries of the colour map plt.imsave applies to rainy_mask (matplotlib's default: viridis). */
int rr_set_colormap(rr_ctx* ctx, const uint8_t* lut_rgba);

/* Render n frames (all with identical H,W,He,We).  Pointers inside `in`/`out` are HOST
 * pointers; the call uploads, renders, downloads and returns after completion. */
int rr_render_frames(rr_ctx* ctx, int32_t n, const rr_frame_in* in, const rr_frame_out* out);

/* Same, but every pointer inside `in`/`out` is a DEVICE pointer on ctx's device.
 * Work is enqueued on `stream` (a hipStream_t; NULL = the ctx's own stream) and the
 * call returns without waiting.  drop_status/arena overflow are checked at
 * rr_synchronize(). */
int rr_render_frames_device(rr_ctx* ctx, int32_t n, const rr_frame_in* in, const rr_frame_out* out, void* stream);
int rr_synchronize(rr_ctx* ctx);

/* ---------------------------------------------------------------------------------------
 * Pre-passes (SURVEY 8f "next" #1, #2): the two image passes that PRODUCE rainy_bg and
 * env_xyY, so that they are born in HBM.  Optional: a caller may keep computing them itself.
 *   fog-like rain attenuation   FogRain.fog_rain_layer           common/add_attenuation.py:88-95
 *   environment map             EnvironmentMapGenerator.generate_map  common/bad_weather.py:742-819
 *                               + convert_rgb_to_xyY              common/generator.py:407-408
 * As with rr_camera, everything derived from transcendentals is computed once by the host. */
#define RR_MAX_TAPS 33
#define RR_PRE_ENV_ONLY 1
#define RR_DEPTH_U16 2
#define RR_DEPTH_PNG_ROWS 3

typedef struct {
  int32_t fog_ksize, env_ksize;   /* 25 (add_attenuation.py:79), 15 (bad_weather.py:815); odd, <= RR_MAX_TAPS */
  double fog_w[RR_MAX_TAPS];      /* cv::getGaussianKernel(25, 25) */
  double env_w[RR_MAX_TAPS];      /* cv::getGaussianKernel(15, 0) -> sigma 2.6 */
} rr_prepass_kernels;

typedef struct {
  int32_t H, W;
  const void* bg;                 /* H*W*3 BGR image / 255 (generator.py:352): float64, or -- in_types -- float32 (RR_IN_BG_F32), or the
                                   * bytes cv2.imread returned (RR_IN_BG_U8: bg = bytes / 255.0 is formed where the kernels read it) */
  const void* depth;              /* H*W metres, float32 (depth_f64 == 0) or float64 (1) (generator.py:362-383) -- or (RR_DEPTH_U16 = 2)
                                   * the uint16 samples of the 16-bit depth PNG as cv2.imread(.., IMREAD_UNCHANGED) returns them:
                                   * metres = sample.astype(float32) / 256 (generator.py:366) is formed where the kernels read it,
                                   * half the upload of the float32 map.  Not with RR_OPT_DEPTH_OCCLUSION. */
  int32_t depth_f64;
  int32_t mode;                   /* 0: fog layer (+ the map if an output asks for it).  RR_PRE_ENV_ONLY (1), rr_prepass_frames*
                                   * only: `bg` IS the fogged image and only the map is made -- the stand-alone
                                   * EnvironmentMapGenerator.generate_map(background) (bad_weather.py:742-819); depth and the fog
                                   * constants are ignored, rr_prepass_out.rainy_bg may be NULL.  One mode per batch. */
  double beta_ext;                /* 0.312 * R**0.67                               add_attenuation.py:40-43 */
  double beta_hg;                 /* Henyey-Greenstein phase term, g = 0.97         add_attenuation.py:60-64 */
  double irr_num, irr_den;        /* 4*N**2  and  exposure_s*gain*pi                add_attenuation.py:51-54 */
  const uint8_t* bg_u8;           /* HOST entry points, kept from version 300: when set, the same as bg = bg_u8 with RR_IN_BG_U8
                                   * (1/8 of the PCIe traffic of the float64 image) */
  int32_t in_types;               /* RR_IN_BG_F32 or RR_IN_BG_U8 (or 0: float64); the other RR_IN_* bits are not for the pre-pass.
                                   * rr_pipeline_* / rr_prepass_frames (host pointers) also take RR_IN_BG_PNG_ROWS: `bg` holds the H rows of
                                   * 1 + 3*W bytes an 8-bit RGB PNG's IDAT stream inflates to (filter type + filtered R G B bytes, as
                                   * rr_io_read_frames_rows delivers them), and depth_f64 = RR_DEPTH_PNG_ROWS: `depth` holds the H rows of
                                   * 1 + 2*W bytes of the 16-bit gray depth file; the filters are reversed on the device.  And RR_IN_BG_JPEG:
                                   * `bg` holds a baseline JPEG's coefficient record (rr_io_read_frames_jpeg; see "Baseline JPEG input frames" below) */
  int32_t reserved;
} rr_prepass_in;

/* Element types of the pre-pass' outputs (rr_prepass_out.out_types).  The pre-pass computes in float64 whatever the
 * types: a float32 output is the float64 result rounded once (what numpy's astype(float32) of the reference's arrays
 * gives), and the uint8 map does not depend on them.  The hot path takes both widths (rr_frame_in.in_types). */
enum { RR_OUT_RAINY_F32 = 1, RR_OUT_ENV_F32 = 2 };

typedef struct {
  void* rainy_bg;                 /* H*W*3: FOG.fog_rain_layer(bg, depth); float64, or float32 with RR_OUT_RAINY_F32 */
  void* env_xyY;                  /* H*We*3, We = cw + 2*(cw/2) (may be NULL); float64, or float32 with RR_OUT_ENV_F32 */
  uint8_t* env_bgr_u8;            /* H*We*3: the map the reference saves with --save_envmap (may be NULL) */
  int32_t out_types;              /* one value for every frame of a batch */
  int32_t reserved;
} rr_prepass_out;

int rr_set_prepass_kernels(rr_ctx* ctx, const rr_prepass_kernels* k);

/* Projection tables of EnvironmentMapGenerator for HxW frames (bad_weather.py:716-762): `uniq` are the
 * n_uniq distinct cylinder cells row*cw+col in ascending order and `first` the source pixel (row*W+col)
 * np.unique(..., return_index=True) pairs with each of them.  Host pointers; copied. */
int rr_set_envmap_geometry(rr_ctx* ctx, int32_t H, int32_t W, int32_t cw, int32_t n_uniq, const int32_t* uniq,
                           const int32_t* first);
int rr_envmap_width(rr_ctx* ctx);                    /* We for the geometry set above, or < 0 */

/* n frames of identical H,W.  DEVICE pointers, enqueued on `stream` (NULL = ctx stream). */
int rr_prepass_frames_device(rr_ctx* ctx, int32_t n, const rr_prepass_in* in, const rr_prepass_out* out, void* stream);
/* HOST pointers: upload, run, download, return after completion. */
int rr_prepass_frames(rr_ctx* ctx, int32_t n, const rr_prepass_in* in, const rr_prepass_out* out);

/* Pre-pass + hot path for n frames with HOST pointers and no host round trip in between:
 * in[f].rainy_bg and in[f].env_xyY are ignored (produced on the device from pre[f]); in[f].bg is ignored
 * too (the mean shift uses pre[f]'s background); in[f].He/We must be H / rr_envmap_width().  pre_out may be NULL, as may each of
 * its members: what is non-NULL is downloaded as well.
 * Width of the arrays handed from the pre-pass to the hot path (they never leave the device unless pre_out asks): what
 * pre_out[].out_types says where pre_out downloads them; otherwise float32 (RR_OPT_PIPELINE_F32, default 1: the mask does
 * not read them, the image contract is +-1 LSB) -- the environment map only when every in[f].omega is NULL (the resident
 * solid angles exist in both widths).  A byte image (bg_u8 / RR_IN_BG_U8) stays bytes on the device. */
int rr_pipeline_frames(rr_ctx* ctx, int32_t n, const rr_prepass_in* pre, const rr_frame_in* in, const rr_frame_out* out,
                       const rr_prepass_out* pre_out);

/* ---------------------------------------------------------------------------------------
 * Render-scale resize of the inputs on the device: full-size frames in.  The frame loader of the reference resizes
 * image / 255 (float64) and the depth map (float32) with cv2.resize(INTER_LINEAR) when a plug-in renders at a fraction of the
 * files' resolution (generator.py:352-381; Cityscapes: render_scale 2).  csrc/rr_resize.h states that resize once -- for
 * rr_io_read_frames_scaled on the host and for the kernels k_resize_in / k_resize_depth -- bit for bit:
 *     f = (k + 0.5) * (s / d) - 0.5;  weight f - floor(f), 0 where floor(f) < 0;  both indices clamped to [0, s - 1]
 *     (a00 (1 - wx) + a01 wx) (1 - wy) + (a10 (1 - wx) + a11 wx) wy      in float64, in this order, not contracted
 * on byte / 255.0 (or the widened float32 value) for the image and on float32(sample) / 256 (or the float32 metres) widened for
 * the depth map, whose result is rounded once to float32.  Equal sizes are the identity.
 *
 * rr_set_input_resize arms the stage with the size of the images (src_H x src_W) and of the depth maps (depth_H x depth_W) the
 * entry points below take from then on; all four 0 disarm it (the context is what it was).  RR_E_ARG for a side outside
 * [1, 16384], RR_E_STATE while a pipeline slot is in flight.  While armed
 *   rr_pipeline_submit / rr_pipeline_frames / rr_prepass_frames (host pointers) read rr_prepass_in.bg as a src_H x src_W image --
 *       RR_IN_BG_U8, bg_u8 or RR_IN_BG_PNG_ROWS (src_H rows of 1 + 3 src_W bytes) -- and depth as a depth_H x depth_W map --
 *       float32, RR_DEPTH_U16 or RR_DEPTH_PNG_ROWS, one kind per batch.  An interleaved float32 / float64 bg, a float64 depth
 *       map and RR_PRE_ENV_ONLY are RR_E_ARG.
 *   rr_augment_frames_device reads images as [n,3,src_H,src_W] and depth as [n,depth_H,depth_W]; rainy_out / mask_out keep H x W.
 * H, W of every descriptor remain the render size.  The stage leaves a float64 B G R image and a float32 depth map of the render
 * size on the device, and the rest of the call is the float64-image route (in_types 0, depth_f64 0) fed those arrays: the same
 * outputs, bit for bit, as the unarmed call given the host-resized arrays.  RR_OPT_DEPTH_OCCLUSION is allowed with every kind of
 * depth input (a float map exists behind the stage).  The source-size inputs wait in a block of the slot's own, sized by the
 * source and allocated by the first armed batch. */
int rr_set_input_resize(rr_ctx* ctx, int32_t src_H, int32_t src_W, int32_t depth_H, int32_t depth_W);
/* The stage alone, on DEVICE arrays, with the sizes of the setter (RR_E_STATE when it is not armed): n images -> bg_out
 * [n,H,W,3] float64 B G R, n depth maps -> depth_out [n,H,W] float32, enqueued on `stream` (NULL: the context's stream, and the
 * call waits for it).  Either side may be NULL.  image_kind: RR_RESIZE_*; depth_kind: 0 (float32 metres) or RR_DEPTH_U16. */
enum { RR_RESIZE_BGR_U8 = 0,             /* [n,src_H,src_W,3] interleaved B G R bytes (the un-filtered file) */
       RR_RESIZE_RGB_U8_PLANAR = 1,      /* [n,3,src_H,src_W] planar R G B bytes */
       RR_RESIZE_RGB_F32_PLANAR = 2,     /* [n,3,src_H,src_W] planar R G B float32: widened, not divided */
       /* rr_tensor_batch's other formats, each the kernel rr_augment_frames_device runs for it while armed.  A frame is
        * src_H * src_W * 3 elements; `images` is aligned to the element size (RR_E_ARG otherwise).  The half types enter as the
        * float32 they widen to exactly (csrc/rr_convert.h). */
       RR_RESIZE_RGB_U8 = 3,             /* [n,src_H,src_W,3] interleaved R G B bytes */
       RR_RESIZE_RGB_F32 = 4,            /* [n,src_H,src_W,3] interleaved R G B float32 */
       RR_RESIZE_RGB_F16_PLANAR = 5,     /* [n,3,src_H,src_W] planar R G B float16 */
       RR_RESIZE_RGB_BF16_PLANAR = 6,    /* [n,3,src_H,src_W] planar R G B bfloat16 */
       RR_RESIZE_RGB_F16 = 7,            /* [n,src_H,src_W,3] interleaved R G B float16 */
       RR_RESIZE_RGB_BF16 = 8 };         /* [n,src_H,src_W,3] interleaved R G B bfloat16 */
int rr_resize_inputs_device(rr_ctx* ctx, int32_t n, int32_t H, int32_t W, const void* images, int32_t image_kind, const void* depth,
                            int32_t depth_kind, double* bg_out, float* depth_out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Particle generator on the device (SURVEY 8f "next" #4, BASELINE.json configs[4]: "in-kernel particle simulation (no
 * XML)").  The reference drives a closed-source simulator binary through tools/simulation.py with the settings of
 * common/db.py:41-70 and reads its output back as XML (bad_weather.py:192-211); there is no source to follow, so the
 * model is this library's own (rain-rendering_amd/tools/particles.py is its bit-exact host statement: Marshall-Palmer
 * sizes, Atlas terminal velocity, exposure-integrated streaks, pinhole projection, counter-based Philox4x32-10 numbers).
 * For every frame the device
 *   1. simulates n_particles streaks (one Philox counter per particle: any particle can be made by any lane),
 *   2. applies the loader's derived fields (bad_weather.py:208-241: render scale, y flip, z sign, widths, ratio, rounding,
 *      length, type) and the frame filter of Generator.run (generator.py:413-420), keeping the particle order,
 *   3. makes the renderer's per-drop random draws (np.random.seed(draw_seed), one randint per drop, one normal per
 *      non-Big drop: bad_weather.py:252-264, generator.py:136) from numpy's legacy MT19937 stream, like rr_host_frame_draws,
 * and leaves rr_drop[] records in HBM: no XML, no host drop table, no PCIe traffic.  Without angular noise the rotation
 * terms are rot_cos = -dy / n, rot_sin = -|dx| / n (n = |end - start|): the values cos / sin(-(theta) * pi / 180),
 * theta = acos(-dy / n), take when evaluated exactly.  Everything derived from transcendentals (the diameter distribution)
 * is tabulated once by the host.
 *
 * Angular noise (--noise_std / --noise_scale, generator.py:136-163): the reference turns the end points of a simulated
 * frame's streaks IN PLACE, so a rendered frame inherits the turns of every earlier frame of the run that used the same
 * simulated frame.  rr_set_particle_noise describes the run; a frame with run_pos = p >= 1 is its entry p - 1 and gets
 * the simulated frame's pristine streaks stepped through every earlier entry with the same `frame`, in run order, then
 * through its own entry: frame filter on the current end points, the entry's draws over the kept streaks (the normal
 * deviate formed with det_log), the kept non-Big streaks turned by (0 + noise_std g) noise_scale degrees about their
 * midpoints (det_sincos; truncated toward zero).  Its records carry the turned end points and the rotation terms
 * cos / sin(-(theta + noise)) of the end points before the turn, as the angle sum of the exact terms above and
 * det_sincos(noise) (tools/particles.py expected_records states it bit for bit).  The context keeps every simulated
 * frame's current state: entries applied in order advance it, an entry older than the state restarts it from the
 * pristine streaks.  State updates follow the order of the calls (an event chains calls on different streams). */
typedef struct rr_sim_frame {
  int32_t sensor_w, sensor_h;     /* cam_CCD_WH (db.py): the simulator's sensor in pixels; rendered frame = sensor / render_scale */
  int32_t render_scale;           /* settings["render_scale"] (bad_weather.py:208-211) */
  int32_t n_particles;            /* streaks simulated for this frame (host: Poisson(expected count), or a fixed count) */
  uint32_t key0, key1;            /* Philox key: the simulation's seed */
  uint32_t frame;                 /* simulated frame number (a word of the Philox counter) */
  uint32_t draw_seed;             /* np.random.seed(...) of the renderer's per-drop draws (generator.py:318) */
  int32_t table;                  /* diameter table of this frame's fall rate / camera (rr_set_particle_tables) */
  int32_t run_pos;                /* angular noise (rr_set_particle_noise): 0 none; p >= 1 this frame is entry p - 1 of the run */
  double fpx;                     /* focal length / pixel size (cam_focal, cam_CCD_pixsize) */
  double exposure_s;              /* cam_exposure / 1000 */
  double speed_mps;               /* sim_steps["cam_motion"] / 3.6 */
  double wind_sigma;              /* m/s, horizontal */
  double margin;                  /* the simulated field exceeds the sensor by this fraction on every side */
  double min_px;                  /* narrowest streak simulated, pixels */
  double z_far;                   /* farthest drop simulated, metres */
} rr_sim_frame;

/* n_tables inverse-CDF tables of the drop diameter (mm): d_grid[n_grid] ascending, cdf[t][n_grid] from 0 to 1,
 * non-decreasing (host pointers, copied).  A diameter is d_grid[j] + (u - cdf[j]) * ((d_grid[j+1] - d_grid[j]) / (cdf[j+1] - cdf[j]))
 * for the j with cdf[j] <= u < cdf[j+1]. */
int rr_set_particle_tables(rr_ctx* ctx, int32_t n_tables, int32_t n_grid, const double* d_grid, const double* cdf);

/* n frames of rendered size H x W: frame f's records go to drops_out + f * cap (DEVICE memory, cap records per frame; what
 * does not fit is not stored) and its drop count to n_out[f] (DEVICE, may exceed cap).  `frames` is a HOST array.  Needs
 * the streak database (texture ratios).  Enqueued on `stream` (NULL = the ctx stream); returns without waiting. */
int rr_generate_drops_device(rr_ctx* ctx, int32_t n, const rr_sim_frame* frames, int32_t H, int32_t W, rr_drop* drops_out,
                             int32_t cap, int32_t* n_out, void* stream);
/* Same with HOST output buffers (n * cap records, n counts): generates on the device, downloads, returns after completion.
 * (A driver that wants the generated particles as data, and the tests.) */
int rr_generate_drops(rr_ctx* ctx, int32_t n, const rr_sim_frame* frames, int32_t H, int32_t W, rr_drop* drops_out, int32_t cap,
                      int32_t* n_out);
int rr_sizeof_sim_frame(void);

/* The run's order for angular noise on device-generated tables: entry p = (simulated frame id run_frame[p] (= the
 * rr_sim_frame.frame of the frames that use it), draw seed run_seed[p]).  Host arrays, copied.  Drops the state the context
 * holds of an earlier run: call it between runs, with no call of the generator in flight.  noise_std or noise_scale 0
 * (or n_run 0) turns the noise off: records are then those of a run without it.  A frame whose run_pos is out of range or
 * names an entry whose frame / seed differ from its own is RR_E_ARG. */
int rr_set_particle_noise(rr_ctx* ctx, double noise_std, double noise_scale, int32_t n_run, const uint32_t* run_frame,
                          const uint32_t* run_seed);

/* The particle model of the records the context generates from now on (every entry point that takes rr_sim_frame records).
 *   RR_PARTICLES_IID (default): every simulated frame draws a fresh, independent set of particles, as described above.
 *   RR_PARTICLES_FIELD: a persistent particle field for video (rain-rendering_amd/tools/particles.py states it bit for bit,
 *     make_field_particles).  A record then reads: n_particles = the run's number of particle SLOTS (about three per
 *     expected particle), frame = the TIME index k of the frame (t = k / cam_hz seconds; it need not wrap with the
 *     simulated frames), every other field as before: the settings in force at that time.  Slot j keeps its diameter and
 *     phase; it lives in the axis-aligned box that bounds the (margin-enlarged) frustum up to z_max(D): half sides
 *     ((1/2 + margin) sensor / fpx) z_max, depth 0 .. z_max, and falls through it once every T = box height / v(D).  Life
 *     g = floor(t / T + phase) is a word of the Philox counter of the life's lateral start, start depth and wind; the
 *     position is the start moved by (wind, -v(D), speed_mps) x the life's age, modulo the box sideways and in depth;
 *     slots outside the frustum are culled.  At any one time the kept particles have the i.i.d. model's law; a particle
 *     kept in frames k and k + 1 in the same life has moved by its velocity / cam_hz.  No state: frame k alone, in any
 *     batch or on any device has the same bits.  A frame's records are in ascending slot order; the per-drop draws
 *     (draw_seed) keep their meaning.  Where two frames' settings differ the field may jump.
 * cam_hz: frames per second (> 0, finite) with RR_PARTICLES_FIELD; ignored (pass 0) with RR_PARTICLES_IID.
 * RR_E_ARG: unknown model, bad cam_hz, or RR_PARTICLES_FIELD while angular noise is on (rr_set_particle_noise with non-zero
 * noise_std and noise_scale; likewise turning the noise on under the field model, or a record with run_pos != 0): the
 * reference's noise turns a shared simulated frame in place and has no meaning for moving particles.
 * Call it between runs, with no call of the generator in flight. */
enum { RR_PARTICLES_IID = 0, RR_PARTICLES_FIELD = 1, RR_PARTICLES_RIG = 2 };
int rr_set_particle_model(rr_ctx* ctx, int32_t model, double cam_hz);

/* RR_PARTICLES_RIG: the field model for a camera rig -- ONE persistent field in the rig's frame seen by up to RR_MAX_VIEWS
 * cameras (stereo, surround; tools/particles.py make_rig_particles states it bit for bit, rain-rendering_amd/rig.py builds
 * the views).  A view is p_cam = R (p_rig - c): R row-major, rig -> camera, orthonormal with determinant +1; c the camera's
 * centre in the rig frame, metres.  The rig frame is the single camera's: x right, y up, looking along -z, drops gain
 * +speed_mps in z.  All views share intrinsics and settings.  box = {r, r_y, o_y} from the host (Rig.box): a slot's box is
 * [-b, b)^2 in x and z, b = r z_max(D), and [-b_y, b_y) in y, b_y = r_y z_max(D) + o_y; x and z wrap modulo 2 b and a
 * view looks at the lattice image nearest to its camera, so r must be at least the horizontal reach of every view's
 * (margin-enlarged) frustum per unit depth.  The records' n_particles and table are the rig's own (rig_slot_counts,
 * rig_tables: density N(D) per unit volume of the box).
 * active[n_active]: the views a batch renders, distinct numbers in 0 .. n_views - 1 (NULL: all n_views in order, n_active
 * ignored).  Under RR_PARTICLES_RIG (rr_set_particle_model(ctx, RR_PARTICLES_RIG, cam_hz), after this call) the batch of
 * every entry point that takes rr_sim_frame records holds n_active consecutive frames per instant: frame i is view
 * active[i % n_active] of instant i / n_active, and the records of one instant agree in every field but draw_seed.  Frame
 * (k, v) is a pure function of (key, k, v): active = {1} gives the tables of view 1 under active = {0, 1}, bit for bit.
 * RR_E_ARG: n_views outside 1 .. RR_MAX_VIEWS; R off orthonormal (an entry of R R^T - I, or det R - 1, beyond 1e-9 in
 * magnitude) or not finite; a bad active list; box values that are not finite, r or r_y not positive, o_y negative; and,
 * when generating: a batch that is not a multiple of n_active, records of one instant that disagree, angular noise,
 * RR_PARTICLES_RIG selected before a rig is set.  Call it between runs, with no call of the generator in flight. */
#define RR_MAX_VIEWS 8
typedef struct {
  double R[9];                    /* rig -> camera, row-major */
  double c[3];                    /* camera centre in the rig frame, metres */
} rr_rig_view;
int rr_set_particle_rig(rr_ctx* ctx, int32_t n_views, const rr_rig_view* views, const double box[3], int32_t n_active,
                        const int32_t* active);
int rr_sizeof_rig_view(void);

/* A camera TRAJECTORY for the rig model: the rig's world (slots, lives, wind, fall, wrap: unchanged) seen from a rig that
 * moves and turns (tools/particles.py make_rig_particles view_end=; rain-rendering_amd/trajectory.py composes the poses).
 * Instant i of the table belongs to time index frame[i] (rr_sim_frame.frame; strictly ascending, any gaps) and holds one
 * rr_traj_pose per view OF THE RIG (n_views of rr_set_particle_rig, not n_active): world -> camera at t_k, p_cam =
 * R0 (p - c0), and at t_k + exposure, (R1, c1); both already composed with the rig's views on the host.  The start of the
 * streak is rr_set_particle_rig's view (R0, c0); its end is R1 ((d + velocity x exposure) - (c1 - c0)) with d the start's
 * wrapped offset: the same lattice image, never wrapped again.  A pose with R1 == R0 and c1 == c0 gives the rig model's
 * bits for the view (R0, c0).  rr_sim_frame.speed_mps stays a drift of the world: pass 0, the trajectory says how the
 * camera moves.  The box of rr_set_particle_rig must hold every pose's frustum (Trajectory.box).
 * Called after rr_set_particle_rig (a later rr_set_particle_rig with another n_views drops the table), between runs, with
 * no call of the generator in flight; the table is copied to the device here, and a batch sends one row number per
 * instant along with its records.  n_instants = 0 turns the trajectory off: the rig model is then exactly what it was.
 * While a table is set, the views' own R and c are not read.  Angular noise stays refused as under the rig model; counter
 * draws and the streak jitter work unchanged.
 * RR_E_ARG: no rig set; frame not strictly ascending; an R off orthonormal (1e-9, as rr_set_particle_rig) or a number that
 * is not finite; |c| > 1e6 m; n_instants > 2^20 (or negative); and, when generating under RR_PARTICLES_RIG, an instant
 * whose rr_sim_frame.frame the table does not hold. */
typedef struct {
  double R0[9], c0[3];            /* world -> camera at t_k: row-major rotation, camera centre (metres) */
  double R1[9], c1[3];            /* the same at t_k + exposure */
} rr_traj_pose;                   /* 192 bytes */
int rr_set_particle_trajectory(rr_ctx* ctx, int32_t n_instants, const uint32_t* frame, const rr_traj_pose* poses);
int rr_sizeof_traj_pose(void);

/* How the per-drop draws of the records the context generates from now on are made (every entry point that takes
 * rr_sim_frame records: rr_generate_drops[_device], rr_frame_in.sim, rr_pipeline_*, rr_augment_frames_device).
 *   RR_DRAWS_STREAM (default): step 3 above -- numpy's legacy stream seeded with draw_seed, replayed by one wave per frame
 *     (k_particle_draws); the records of a run that writes the reference's files.
 *   RR_DRAWS_COUNTER: the texture pick comes from the drop's own Philox counter, and the generator writes the final
 *     tex_index itself (no k_particle_draws):
 *         pick = (w * 10) >> 32 in 64-bit, w = word 2 of the drop's Philox block 1 -- counter (i, frame, 1, 0) under
 *         RR_PARTICLES_IID, the life's block (j, g_lo, 1, 2 + g_hi) under RR_PARTICLES_FIELD and RR_PARTICLES_RIG: a word the
 *         generator computes anyway and no other draw reads;
 *         tex_index = 10 * texture_bucket(ratio) + pick.
 *     Under the field and rig models the pick is a function of (key, slot, life): the same in every frame of a drop's life
 *     and in every view of the rig.  (The ratio bucket comes from the projected size and can still differ between frames
 *     or views.)  Under the i.i.d. model it is a function of (key, frame, particle index).  draw_seed is ignored.  Every
 *     other field of a record is the stream mode's (tools/particles.py expected_records(draws='counter') states it).
 * RR_E_ARG: unknown mode; RR_DRAWS_COUNTER while angular noise is on (the noise needs the stream's normal deviates and run
 * order), likewise turning the noise on under RR_DRAWS_COUNTER (rr_set_particle_noise), or a record with run_pos != 0.
 * Call it between runs, with no call of the generator in flight. */
enum { RR_DRAWS_STREAM = 0, RR_DRAWS_COUNTER = 1 };
int rr_set_particle_draws(rr_ctx* ctx, int32_t mode);

/* Streak jitter: every drop of the records the context generates from now on gets a tilt of its own (every entry point that
 * takes rr_sim_frame records, every particle model, both draw modes).  It is NOT the reference's angular noise
 * (rr_set_particle_noise), whose deviates come from a run's sequential stream: here
 *     g = sqrt(-2 det_log(u1)) cos(2 pi u2)   -- Box-Muller on the drop's Philox block 3 under the frame's key: counter
 *         (i, frame, 3, 0) under RR_PARTICLES_IID, the life's block (j, g_lo, 3, 2 + g_hi) under RR_PARTICLES_FIELD and
 *         RR_PARTICLES_RIG (no other draw reads a block 3); u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) 2^-53 in (0, 1],
 *         u2 = (w2 + 1/2) 2^-32; a standard normal deviate, |g| < 8.6;
 *     after the derived fields and the frame filter (both on the unturned end points) every kept non-Big record is turned by
 *     jitter_deg * g degrees the way the angular noise turns one: rotation terms cos / sin(-(theta + angle)) by the angle sum
 *     with det_sincos, end points about their midpoint, truncated toward zero.  Big drops are untouched.
 * The kept set, the counts, length, max_width, tex_index and the world positions do not depend on it; a streak turned to zero
 * length gets NaN rotation terms, as under the angular noise.  Under the field and rig models g is a function of
 * (key, slot, life): a drop keeps its tilt in every frame of its life and in every view of the rig.  The particle kernels do
 * it themselves (kept lanes only): no further launch.  tools/particles.py expected_records(jitter=) states the records bit
 * for bit.  jitter_deg = 0 (default): off, the records and the kernels are those without it.
 * RR_E_ARG: jitter_deg negative or not finite; a non-zero jitter while angular noise is on, likewise turning the noise on
 * (rr_set_particle_noise) while the jitter is on; and, when generating with the jitter on, a record with run_pos != 0.
 * rr_augment_frames_device accepts a context with the jitter on.  Call it between runs, with no call of the generator in
 * flight. */
int rr_set_particle_jitter(rr_ctx* ctx, double jitter_deg);

/* Mean wind: the air's mean horizontal velocity (wx, wz) in m/s for the records the context generates from now on (every entry
 * point that takes rr_sim_frame records, every particle model, both draw modes, with or without jitter, rig or trajectory), in
 * the axes of the particle world: x right, z toward the viewer -- the camera frame under RR_PARTICLES_IID and
 * RR_PARTICLES_FIELD, the rig frame under RR_PARTICLES_RIG, the lattice's world frame under a trajectory (a rig yawed by 90
 * degrees sees wx along its own z).  It is added to a drop's horizontal velocity, once:
 *     vx = wind_life + wx,  vz = speed_mps + wz        -- one IEEE double addition each, no contraction
 * and (vx, vz) take the place of the life's wind (block_wind, the zero-mean scatter of wind_sigma) and of
 * rr_sim_frame.speed_mps wherever those enter: the streak's end under every model, and the position inside a life under the
 * field and rig models (qx = u + vx tau / w_box, qz = u -/+ vz tau / depth-of-box; a translation modulo the box keeps the
 * uniform law, so a single frame of the field still follows the i.i.d. model's law).  Slot counts, boxes, lives, tables, the
 * texture pick and the jitter's deviate do not depend on it.  A drop of terminal velocity v falls at atan(wx / v) to the
 * vertical: small drops lean more than large ones.  The renderer draws such streaks correctly only with RR_OPT_STREAK_LEAN.
 * The particle kernels take the two numbers as arguments: no further launch.  tools/particles.py expected_records(wind=)
 * states the records bit for bit.  (0, 0) (default): off -- the records and the kernels are those without it (the sums are
 * not formed: x + 0.0 is not x for x = -0.0).  Angular noise stays where it is allowed today (RR_PARTICLES_IID).
 * Not simulated: a streak that starts outside the margin-enlarged field and ends inside it (as for speed_mps); a vertical
 * wind.  One mean wind per context; a wind that changes over time is rr_set_particle_gusts.
 * RR_E_ARG: a component that is not finite or whose magnitude exceeds 100 m/s.  Call it between runs, with no call of the
 * generator in flight. */
int rr_set_particle_wind(rr_ctx* ctx, double wx, double wz);

/* Gusts: a wind that changes over time, under RR_PARTICLES_FIELD and RR_PARTICLES_RIG (with or without a trajectory, both draw
 * modes, with or without jitter), on top of the mean wind.  disp = G[0 .. n]: (n + 1) x 2 doubles, row i the air's horizontal
 * DISPLACEMENT (x, z) in metres at time index frame0 + i, in the mean wind's axes; the air moves linearly between samples.  The
 * table is the caller's (tools/particles.py gust_series makes an Ornstein-Uhlenbeck one); the device looks up, interpolates and
 * adds -- no transcendental, no state.  With m = rr_sim_frame.frame - frame0 and back = tau cam_hz (tau: seconds since the
 * drop's life began), every step one IEEE double operation, no contraction:
 *     sb = m - back;  i = max(floor(sb), 0);  Gb = G[i] + (sb - i) (G[i + 1] - G[i])
 *     dG = G[m] - Gb;  ge = (G[m + 1] - G[m]) cam_hz
 * (before the series starts the first interval's velocity is held).  dG joins the mean wind's term in the position of a life,
 * (vx tau + dGx) / w_box, and ge its velocity in the streak's end, vx + gex; with a series set both mean-wind additions are
 * formed, also for a mean of (0, 0).  Under the rig model the term is evaluated once per slot, for every view; under a
 * trajectory it is a world-frame vector.  Slot counts, boxes, lives, tables, the pick and the jitter do not depend on it, and a
 * single frame keeps the i.i.d. law.  Drops follow the air with no inertia.  tools/particles.py expected_records(gusts=) states
 * the records bit for bit.  The table is uploaded here, once; the particle kernels read it and take no further launch.
 * Call it after rr_set_particle_model (it needs cam_hz; a later rr_set_particle_model drops the series), between runs, with no
 * call of the generator in flight.  n = 0 turns gusts off: the context is what it was.  One series per context.
 * RR_E_ARG when setting: n < 0 or n > 2^20; frame0 + n > 2^32; a number that is not finite; |G| > 1e6 m; an interval whose
 * |step| cam_hz exceeds 100 m/s; the model is RR_PARTICLES_IID (rr_set_particle_model to RR_PARTICLES_IID while a series is set
 * is refused likewise).  RR_E_ARG when generating: a record whose frame lies outside [frame0, frame0 + n); run_pos != 0. */
int rr_set_particle_gusts(rr_ctx* ctx, int32_t n, uint32_t frame0, const double* disp /* (n + 1) x 2, metres */);

/* Showers: a rain rate that changes over time, under RR_PARTICLES_FIELD and RR_PARTICLES_RIG (with or without a trajectory, both
 * draw modes, with or without jitter, wind and gusts).  The slots, tables and capacities of the run are those of the series' PEAK
 * rate; a life of a slot is kept with the probability N(D; R) / N(D; R_peak) = exp(-(Lambda(R) - Lambda(R_peak)) D) of the rate R at
 * the life's BIRTH (Marshall-Palmer, Lambda = 4.1 R^-0.21 mm^-1): the peak's field thinned to the lower rate, in law the field at
 * rate R, and a drop that has started to fall keeps falling.  dlam = L[0 .. n]: n + 1 doubles, L[i] = min(Lambda(rate at time index
 * frame0 + i) - Lambda(peak), 100) mm^-1 (a rate of 0: 100), linear between samples.  The table is the caller's
 * (tools/particles.py RateSeries.dlam; shower_series makes a series); the device looks up, interpolates and compares -- no state.
 * With m = rr_sim_frame.frame - frame0, tau the seconds since the life began and D its diameter in mm, every step one IEEE
 * double operation, no contraction:
 *     sb = max(m - tau cam_hz, 0);  i = floor(sb);  Lb = L[i] + (sb - i) (L[i + 1] - L[i]);  p = det_exp(-(Lb D))
 *     alive = unit32(w) < p            w: word 3 of the life's Philox block 1, which nothing else reads
 * (before the series starts its first value is held).  A life that is not alive is culled as a slot outside the frustum is; under
 * the rig model the decision is made once per slot, for every view.  L = 0 gives p = 1 exactly: a series at its peak leaves the
 * records of no series, byte for byte.  L = 100 gives p < 2^-33, unit32's smallest value: no new drop.  Slot counts, boxes, lives,
 * tables, positions, the pick, the jitter, wind and gusts do not depend on it.  tools/particles.py expected_records(rate_series=)
 * states the records bit for bit.  The table is uploaded here, once; the particle kernels read it and take no further launch.
 * Call it after rr_set_particle_model (a later rr_set_particle_model drops the series), between runs, with no call of the generator
 * in flight.  n = 0 turns it off: the context is what it was.  One series per context.
 * RR_E_ARG when setting: n < 0 or n > 2^20; frame0 + n > 2^32; a value that is not finite, below 0 or above 100; the model is
 * RR_PARTICLES_IID (rr_set_particle_model to RR_PARTICLES_IID while a series is set is refused likewise).  RR_E_ARG when
 * generating: a record whose frame lies outside [frame0, frame0 + n); run_pos != 0. */
int rr_set_particle_rate_series(rr_ctx* ctx, int32_t n, uint32_t frame0, const double* dlam /* n + 1, mm^-1 */);

/* ---------------------------------------------------------------------------------------
 * Rain on a batch of images that already lives on the GPU in a deep-learning framework's layout (PyTorch: planar RGB,
 * [n][3][H][W], bytes or float32 in [0, 1]) -- rain-rendering_amd/augment.py RainAugment.  One call enqueues on `stream`
 * (NULL = the ctx stream)
 *     particles (rr_generate_drops_device semantics: tables and counts stay on the device)
 *  -> ingest (k_planar_in, or k_tensor_in for the formats behind planar bytes and float32: the caller's RGB -> the interleaved
 *     BGR image, RR_IN_BG_U8 / RR_IN_BG_F32; values moved, a float16 / bfloat16 element widened to the float32 it equals exactly,
 *     subnormals included)
 *  -> pre-pass (fog layer + xyY map handed over as float32, the resident solid angles: rr_pipeline_frames' defaults)
 *  -> hot path -> finalize (k_finalize_planar: rainy_out in the images' layout and dtype, mask_out = float(mask_f64))
 * and then waits on `stream` for the 4-byte arena-overflow flag: when the tile arena had to grow, the batch is enqueued once more.
 * So the call returns after the batch is complete -- a host wait on the caller's stream.  For the same records and input values
 * the result is bit for bit what rr_pipeline_frames gives: rainy_out bytes == rainy_rgb (planar), float32 rainy_out == those
 * bytes / 255.0f (what ToTensor makes of the PNG the driver writes), float16 / bfloat16 rainy_out == that float32 rounded once to the
 * half type, to nearest, ties to even (csrc/rr_convert.h).  layout (RR_LAYOUT_*) only moves values: the interleaved result of a
 * batch is, element for element, the planar result of the same values, and mask_out depends on neither dtype nor layout.  All eight
 * (dtype, layout) pairs work with and without an armed rr_set_input_resize (the half types feed (double)value, as float32 does).
 * RR_E_ARG, with nothing enqueued: a dtype outside {RR_TENSOR_U8, RR_TENSOR_F32, RR_TENSOR_F16, RR_TENSOR_BF16}, a layout outside
 * {RR_LAYOUT_PLANAR, RR_LAYOUT_INTERLEAVED}, images or rainy_out not aligned to the element size.
 * Not offered: angular noise (run_pos must be 0; the streak jitter of rr_set_particle_jitter is), the 'white' strategy, opacity attenuation.  Needs the streak database, camera, pre-pass kernels, particle tables, the envmap geometry of
 * H x W and the solid angles of the H x rr_envmap_width() map (rr_set_solid_angles).  The caller's current device is restored.
 * Scratch in the context, grown to the largest batch seen and never shrunk, per frame about
 *     3 H W (bytes; 12 H W for float32, float16 and bfloat16, which ingest into the float32 image; 24 H W for any dtype while
 *     rr_set_input_resize is armed, plus 4 H W where the depth map is resized)
 *     + 12 H W (fog layer) + 12 H We (map) + 8 H W (mask) + 112 drops_cap  bytes
 * (KITTI 1242 x 375 with bytes: about 23 MB per frame) on top of the hot path's own per-batch scratch. */
enum { RR_TENSOR_U8 = 0, RR_TENSOR_F32 = 1,
       RR_TENSOR_U8_HWC = 3,             /* interleaved bytes [n,H,W,3]: rr_lens_batch.dtype only (rr_augment_frames_device refuses it:
                                          * there the layout is rr_tensor_batch.layout).
                                          * 2 names no layout and stays refused everywhere, as it was before this layout existed */
       RR_TENSOR_F16 = 4,                /* IEEE binary16; rr_tensor_batch.dtype only */
       RR_TENSOR_BF16 = 5 };             /* bfloat16; rr_tensor_batch.dtype only */
enum { RR_LAYOUT_PLANAR = 0,             /* [n,3,H,W] */
       RR_LAYOUT_INTERLEAVED = 1 };      /* [n,H,W,3] RGB: pixel p's channel c at element 3 p + c (a channels-last tensor) */
typedef struct {
  int32_t n, H, W, dtype;                /* dtype: RR_TENSOR_*; images and rainy_out share it and the layout */
  const void* images;                    /* DEVICE, RGB in `layout`, contiguous: bytes, or float32 / float16 / bfloat16 in [0,1] */
  const float* depth;                    /* DEVICE, [n,H,W] metres */
  const struct rr_sim_frame* sims;       /* HOST, n records (frame, draw_seed, table, ...) */
  const double* fog;                     /* HOST, n x the four pre-pass constants (beta_ext, beta_hg, irr_num, irr_den) */
  int32_t drops_cap;                     /* drop-table capacity per frame */
  int32_t layout;                        /* RR_LAYOUT_* (0, what a zeroed struct has always said: planar) */
  void* rainy_out;                       /* DEVICE, RGB in `layout`, same dtype as images */
  float* mask_out;                       /* DEVICE, [n,H,W]: float32(rainy_mask) */
} rr_tensor_batch;
int rr_augment_frames_device(rr_ctx* ctx, const rr_tensor_batch* b, void* stream);
int rr_sizeof_tensor_batch(void);

/* ---------------------------------------------------------------------------------------
 * Drops on the lens: adherent raindrops on the camera's lens or windshield, on a batch of planar images that lives on the GPU
 * (rain-rendering_amd/augment.py RainAugment(lens=) and LensAugment).  The reference has nothing of the kind: the
 * model is this library's own, stated bit for bit by rain-rendering_amd/tools/lens.py apply_numpy, its arithmetic by
 * csrc/rr_lens.h.  Every drop is a small inverted, minified, defocused view of the INPUT image with a soft edge and a dark rim.
 * For pixel (x, y) of a drop's bounding box floor(cx - rx) .. floor(cx + rx) + 1 (likewise y), clipped to the frame, in double:
 *     u = (x - cx) / rx, v = (y - cy) / ry, rho2 = u u + v v
 *     t = clamp((1 - rho2) / edge, 0, 1), A = float(t t (3 - 2 t))               coverage; A == 0: the input value, bit for bit
 *     g = 1 / sqrt(1 - 0.75 min(rho2, 1)), sx = cx - (mag (x - cx)) g, sy alike    clamped to the frame; upside down and mirrored
 * and in float, every step one IEEE operation, no contraction:
 *     V(q)   bilinear sample of the input at (sx, sy) between floor(s) and min(floor(s) + 1, size - 1), fractions float(s - floor(s))
 *     B      the separable blur of V with the 2 R + 1 weights of the drop's class, rows then columns, taps added in ascending
 *            offset order, V evaluated at q clamped to the frame
 *     out = (1 - A) in + A (float(1 - (rim rho2) rho2) B)
 * Pixel values enter as float(value): 0 .. 255 for bytes, which store clamp(rint(out), 0, 255) (half to even); float32 stores out.
 * Every drop refracts `images`, never `out`, and the bounding boxes of one frame's drops must be pairwise disjoint, so the result
 * does not depend on any order.  alpha_out (may be NULL) receives A inside the boxes and 0 elsewhere.
 *
 * rr_lens_drops_device enqueues on `stream` (NULL = the ctx stream): the device-to-device copy images -> out (and the clearing of
 * alpha_out), the upload of the records, the blur table and the work list (one workgroup per 32 x 32 piece of a box) through the
 * context's pinned ring, and ONE kernel, k_lens_drops.  counts, drops, class_radius and weights are read before the call returns.
 * With a stream of the caller's it returns without waiting; with NULL it waits for the context's stream (the caller has no handle
 * to order later work behind it).  The caller's current device is restored.
 * RR_E_ARG, with nothing enqueued: a null pointer, sizes or dtype out of range; out or alpha_out overlapping images or each other;
 * a count above cap or RR_MAX_LENS_DROPS; a field that is not finite; rx or ry <= 0; mag < 1; edge outside (0, 1]; rim outside
 * [0, 1]; sigma_class not an integer in 0 .. n_classes - 1; n_classes outside 1 .. 16, a class radius outside 0 .. 15 or a
 * weight that is not finite; two overlapping bounding boxes in one frame. */
#define RR_MAX_LENS_DROPS 128
typedef struct {
  float cx, cy;                          /* centre, pixels */
  float rx, ry;                          /* semi-axes, pixels, > 0 */
  float mag;                             /* how many times wider the field seen through the drop is, >= 1 */
  float edge;                            /* soft-edge width, (0, 1] */
  float rim;                             /* rim darkening, [0, 1] */
  float sigma_class;                     /* blur class: a float holding an integer in 0 .. n_classes - 1 */
} rr_lens_drop;                          /* 32 bytes */
typedef struct {
  int32_t n, H, W, dtype;                /* dtype: RR_TENSOR_*; images and out share it */
  const void* images;                    /* DEVICE, [n,3,H,W] planar, contiguous */
  void* out;                             /* DEVICE, [n,3,H,W]; must not overlap images */
  float* alpha_out;                      /* DEVICE, [n,H,W], or NULL */
  const int32_t* counts;                 /* HOST, n drop counts */
  const rr_lens_drop* drops;             /* HOST, n x cap records: frame f's are drops[f * cap .. f * cap + counts[f]) */
  int32_t cap;
  int32_t n_classes;                     /* 1 .. 16 */
  const int32_t* class_radius;           /* HOST, n_classes radii R in 0 .. 15 */
  const float* weights;                  /* HOST, 16 x 31 float32: class c's 2 R + 1 taps are weights[31 c .. 31 c + 2 R] */
} rr_lens_batch;
int rr_lens_drops_device(rr_ctx* ctx, const rr_lens_batch* b, void* stream);
int rr_sizeof_lens_drop(void);
int rr_sizeof_lens_batch(void);
/* rr_lens_batch.dtype == RR_TENSOR_U8_HWC: images and out are [n,H,W,3] interleaved bytes (pixel p's channel c at byte 3 p + c, the
 * layout of rr_frame_out.rainy_rgb); alpha_out stays float32 [n,H,W].  The same arithmetic, byte for byte what RR_TENSOR_U8 gives on
 * the transposed planes.
 *
 * Drops on the lens inside the frame pipeline.  rr_pipeline_set_lens ARMS a pipeline slot: every batch submitted on it
 * afterwards (rr_pipeline_submit; slot 0 also serves rr_pipeline_frames and rr_render_frames) runs the lens pass between the
 * finalize kernel and the PNG rows, so rainy_rgb and rainy_png carry the drops of frame f's table.  rainy_bg_out, mask_f64, mask_i32,
 * mask_png, drop_status and drop_colour are what they are without it: the streak mask knows nothing of the lens.  The armed state stays
 * on the slot until it is replaced or disarmed (lens == NULL), and EVERY submit on the slot applies it once -- the re-submit after
 * RR_E_ARENA included, so the batch that is submitted again gets its drops once, not twice.
 *   counts, drops, class_radius, weights   HOST pointers with the meaning and the checks of rr_lens_batch; copied before the call returns
 *   alpha_png     NULL, or n HOST pointers, each NULL or a buffer of H * (1 + 4 W) bytes that receives the frame's LABEL file the way
 *                 mask_png receives the mask file: PNG scanlines (filter Sub) of RGBA pixels R = G = B = v, alpha 255, with
 *                 v = clamp(rint(A * 255.0f)) (half to even; A the coverage, 0 outside the drops) -- or, under RR_OPT_PNG_DEFLATE, the
 *                 finished zlib stream behind the 16-byte header (same rule, same fallback).  The buffers must stay valid until
 *                 rr_pipeline_wait of every batch submitted while the slot is armed with them.
 * Device memory of an armed slot, allocated by the call and kept: n H W 4 bytes (the un-dropped copy of the frames and the label
 * plane) plus n H (1 + 4 W) for the label's scanlines when alpha_png asks for them.
 * RR_E_ARG, with nothing changed: a bad slot, n, H or W <= 0, a null table, or any table error of rr_lens_drops_device's list.
 * RR_E_STATE: the slot is in flight.  rr_pipeline_submit on an armed slot returns RR_E_ARG with nothing enqueued when the batch's n, H
 * or W are not the armed ones or when the batch renders nothing (in == NULL; rr_prepass_frames runs on slot 0). */
typedef struct {
  int32_t n, H, W, cap;
  const int32_t* counts;                 /* HOST, n drop counts */
  const rr_lens_drop* drops;             /* HOST, n x cap records */
  int32_t n_classes, reserved;
  const int32_t* class_radius;           /* HOST */
  const float* weights;                  /* HOST, 16 x 31 float32 */
  uint8_t* const* alpha_png;             /* NULL, or n HOST pointers (each may be NULL) */
} rr_pipeline_lens;
int rr_pipeline_set_lens(rr_ctx* ctx, int32_t slot, const rr_pipeline_lens* lens);
int rr_sizeof_pipeline_lens(void);

/* ---------------------------------------------------------------------------------------
 * The rain layer of a frame (kernel and contract: csrc/rr_layer.h): what the streaks add to a pixel and how much of
 * the background survives under them -- the third thing, beside the rainy frame and the rain-free target, that de-raining,
 * rain-removal and rain-segmentation models are trained on.  rainy_mask is not it: an unbounded sum of alpha samples, no colour.
 * For pixel p of frame f take the drops the compositor lists for p, in table order; A is the drop's alpha sample at p, 0 outside
 * its footprint and, under RR_OPT_DEPTH_OCCLUSION, 0 where the drop is behind the scene (the compositor's rule).  Start with
 * T = 1, L = (0, 0, 0); per drop
 *     u = 1 - A te;   L_c <- u L_c + A kg_c  (c = B, G, R);   T <- u T              no clamp anywhere
 * te = tau_one / exposure and kg_c = K_c g being the drop's blend factors as the colour kernel leaves them, rounded to float32.
 * The device carries T and L in float32, one IEEE operation per step: Af = float(A), u = fma(Af, -te, 1),
 * L_c = fma(u, L_c, Af * kg_c), T = u * T.  A drop whose factors are not tame, or whose tile is the caller's (rr_ext_tile), takes
 * the float64 factors and makes the step in float64 on double(L_c), double(T), rounding each result once to float32.
 * A pixel no listed drop reaches has T == 1 and L == 0 exactly.  T and L depend on neither bg nor rainy_bg, nor on which compositor
 * made the image (float or float64 colours, RR_OPT_WILD_PIXELS, RR_OPT_COLOUR_STREAM); the colour constants follow RR_OPT_FOV_F32.
 *   layer   float32 [H][W][4] = (L_B, L_G, L_R, T): 16 bytes per pixel, the pointer 16-byte aligned
 *   shift   one double: the mean shift every finalize kernel subtracts, mean(composite) - mean(bg) of the frame
 * Wherever no blend of the compositor clamped, the composite is T rainy_bg + L, so
 *     rainy_rgb = uint8(clip01(T rainy_bg + L - shift) 255)                            within 1 LSB
 * Sufficient for "no blend clamped": bg and rainy_bg lie in [0, 1] and kg_c <= te for every listed drop (each blend is then a
 * convex combination).  The layer knows nothing of the lens pass (rr_pipeline_set_lens), exactly like the mask.
 *
 * rr_pipeline_set_layer ARMS a pipeline slot, modelled on rr_pipeline_set_lens: every batch submitted on it afterwards
 * (rr_pipeline_submit; slot 0 also serves rr_pipeline_frames, rr_render_frames and rr_render_frames_device) runs ONE more kernel
 * beside the compositor, k_rain_layer, over the compositor's own work lists, and a one-workgroup-per-frame kernel for the shift.
 * frames[f] says where frame f's layer and shift go; either pointer may be NULL.  The pointers are of the kind the consuming
 * entry point takes: HOST for the host-pointer entry points (they must stay valid until rr_pipeline_wait of every batch submitted
 * while the slot is armed with them), DEVICE for rr_render_frames_device.  The table is copied by the call.  The armed state stays
 * on the slot until it is replaced or disarmed (layer == NULL), and EVERY submit on the slot applies it once, the re-submit after
 * RR_E_ARENA included.  With no layer armed the kernels of a call are what they were: nothing else changes.
 * Device staging of the host entry points, allocated by the first armed batch and kept: 16 H W + 8 bytes per frame.
 * RR_E_ARG, with nothing changed: a bad slot, n <= 0, a null table (frames), a layer pointer that is not 16-byte aligned.
 * RR_E_STATE: the slot is in flight.  A submit on an armed slot returns RR_E_ARG with nothing enqueued when the batch's n is not the
 * armed n or when the batch renders nothing (in == NULL; rr_prepass_frames runs on slot 0). */
typedef struct {
  float* layer;                          /* [H][W][4] float32 (L_B, L_G, L_R, T), or NULL */
  double* shift;                         /* one double, or NULL */
} rr_layer_out;                          /* 16 bytes */
typedef struct {
  int32_t n, reserved;
  const rr_layer_out* frames;            /* HOST, n records */
} rr_pipeline_layer;
int rr_pipeline_set_layer(rr_ctx* ctx, int32_t slot, const rr_pipeline_layer* layer);
int rr_sizeof_layer_out(void);
int rr_sizeof_pipeline_layer(void);
/* The rain layer as a FILE: rr_pipeline_set_layer_png ARMS a pipeline slot so that every batch submitted on it
 * afterwards also leaves each frame's layer as the payload of a straight-alpha 8-bit RGBA PNG -- what rainy_png is for the image: H rows
 * of 1 + 4 W bytes, filter type 1 (Sub), or under RR_OPT_PNG_DEFLATE the RRZ1 stream -- for rr_png_write_scanlines /
 * rr_io_write_frames_text.  From a pixel's float32 (L_B, L_G, L_R, T):
 *     a  = 1.0f - T                                   (float32)
 *     A8 = clamp(rint(a * 255.0f), 0, 255)            (float32 multiply, half to even, NaN -> 0)
 *     A8 == 0: R = G = B = 0;  else C_c = clamp(rint(double(L_c) * (65025.0 / double(A8))), 0, 255)   (NaN -> 0; c = R, G, B)
 *     file pixel = (C_R, C_G, C_B, A8)
 * The reader's T' = 1 - A8 / 255 and L'_c = A8 C_c / 65025 (PNG's `over` with the file's own numbers is T' x + L').  Wherever
 * 0 <= T <= 1 and 0 <= L_c <= 1 - T -- which holds when kg_c <= te for every listed drop -- |T' - T| and |L'_c - L_c| are at most
 * 1 / 510 plus the float32 rounding of a * 255, so |T' x + L' - (T x + L)| <= 1 / 255 for x in [0, 1].
 *   layer_png   n HOST pointers, each NULL or a buffer of H * (1 + 4 W) bytes; downloaded by rr_pipeline_wait with the batch's other
 *               outputs, exactly as rr_pipeline_lens.alpha_png is.  The table is copied by the call.
 * The kernels: k_rain_layer's byte-store variant (the same walk, once; it also stores the float layer where rr_pipeline_set_layer
 * armed one on the slot -- the two armings are independent) and k_png_layer for the Sub filter; under RR_OPT_PNG_DEFLATE the layer is
 * one more stream of the device coder.  Armed until replaced or disarmed (NULL); every submit on the slot applies it once, the
 * re-submit after RR_E_ARENA included; slot 0 also serves rr_pipeline_frames / rr_render_frames.  With nothing armed the kernels of a
 * call are what they were.  Device staging, allocated by the first armed batch and kept: 4 H W bytes per frame for the RGBA pixels
 * plus H (1 + 4 W), rounded up to 16, for the scanlines.
 * RR_E_ARG, with nothing changed: a bad slot, n, H or W <= 0, a null table.  RR_E_STATE: the slot is in flight.  A submit on an armed
 * slot returns RR_E_ARG with nothing enqueued when the batch's n, H or W are not the armed ones or when the batch renders nothing
 * (in == NULL); so does rr_render_frames_device while slot 0 is armed: the file route is the host entry points'. */
typedef struct {
  int32_t n, H, W, reserved;
  uint8_t* const* layer_png;             /* n HOST pointers (each may be NULL) */
} rr_pipeline_layer_png;                 /* 24 bytes */
int rr_pipeline_set_layer_png(rr_ctx* ctx, int32_t slot, const rr_pipeline_layer_png* layer_png);
int rr_sizeof_pipeline_layer_png(void);
/* The same for rr_augment_frames_device: armed until replaced or disarmed (layer == NULL, or all three pointers NULL), every call
 * (its re-enqueue after an arena growth included) fills, for its n frames at its H x W -- the render size under rr_set_input_resize --,
 *   layer_out        DEVICE [n,4,H,W] planar float32 in the order R, G, B, T (L_R, L_G, L_B, T), or NULL
 *   background_out   DEVICE [n,3,H,W] planar float32 RGB, or NULL: the fogged image the streaks were composited over -- the
 *                    pre-pass output the hot path read, the float32 values themselves, not re-quantised
 *   shift_out        DEVICE [n] double, or NULL
 * always planar float32, whatever dtype and layout the images have (as mask_out is always float32).  The planes are written by a
 * store variant of the same kernel: the lists are walked once.  No scratch of the library's: the caller's tensors are written
 * directly.  RR_E_ARG: a pointer that is not aligned to its element. */
typedef struct {
  float* layer_out;
  float* background_out;
  double* shift_out;
} rr_tensor_layer;
int rr_augment_set_layer(rr_ctx* ctx, const rr_tensor_layer* layer);
int rr_sizeof_tensor_layer(void);

/* Options.  Those marked "tuning" change no result bit (tests/test_gpu_properties.py); every other one says what it
 * changes.  A retired option keeps its number and accepts only the value the library always runs with (it then does
 * nothing).  Unknown options or values are RR_E_ARG.  The library reads no environment variables. */
enum {
  RR_OPT_DEDUP = 1,                 /* tuning: 1 (default): drops with bit-identical raw-tile parameters share one tile inside a batch */
  RR_OPT_GENERAL_FOV = 2,           /* 1: force the general colour path (prefix table in HBM) that maps taller than 1024 rows,
                                     *    wider than 4096 columns or with He*We >= 2^22 always take; default 0.  The colour sums
                                     *    are added in another order: rainy_image within 1 LSB, mask and statuses the same */
  RR_OPT_FOV_THREADS = 3,           /* retired: only 0 or 1024 is accepted */
  RR_OPT_FOV_DROPS_PER_THREAD = 4,  /* tuning: drops per thread of the FOV-sum kernel: 0 (library's choice), 1, 2, 4 or 8 */
  /* NOT a tuning switch -- a feature the reference only sketches (common/drop_depth_map.py, dead code behind
   * USE_DEPTH_WEIGHTING = 0, generator.py:20): with 1, a drop is not composited at pixels whose scene depth
   * (rr_frame_in.depth / the pre-pass' depth) is smaller than the drop's distance |world z|.  Default 0: the reference's
   * output.  Excluded from every parity run. */
  RR_OPT_DEPTH_OCCLUSION = 5,
  RR_OPT_BLUR_WORKGROUPS = 6,       /* retired: only 0 or 4 is accepted */
  /* Colour arithmetic of the compositor.  rainy_mask is a float64 sum in drop order in either case (bit-exact); the three
   * colour channels of rainy_image only have to land within 1 LSB of a uint8 (BASELINE.json), so by default they are
   * blended in float whenever no frame of the batch asks for the float64 composite (rr_frame_out.rainy_bg_out == NULL).
   * 1: float64 colours always (the reference's arithmetic; what rainy_bg_out != NULL gets anyway).  The uint8 image of
   * the two differs by at most 1 LSB (tests/test_gpu_properties.py). */
  RR_OPT_COMPOSITE_F64 = 7,
  /* tuning: how the host-pointer entry points move a batch across PCIe.  0 (default): hipMemcpyAsync (the DMA engines),
   * after merging neighbouring pieces -- frames laid out back to back in one rr_host_alloc block, each starting on a
   * 16-byte boundary, travel as ONE copy per array (so a gap of fewer than 16 bytes between two consecutive frames'
   * arrays of one kind inside such a block is treated as padding: uploads read it, downloads may overwrite it).  1: the pieces whose host side is page-locked and 16-byte aligned are
   * moved by one copy kernel per direction that reads / writes the host memory directly (faster than many small DMA
   * requests -- 90 vs 40 GB/s both ways, scripts/probes/pcie_probe.hip -- but it takes compute units from the rendering
   * kernels it runs beside: measured slower end to end). */
  RR_OPT_COPY_KERNELS = 8,
  RR_OPT_PADDED_TEXTURES = 9,       /* retired: only 1 is accepted */
  /* precision of the colour branch: 0 float64 throughout (the reference's arithmetic), 1 float32 always, 2 (default) float32
   * whenever the compositor blends float colours (no frame of the batch asks for the float64 composite: the same switch as
   * RR_OPT_COMPOSITE_F64's default).  Float32 = the field-of-view vertices (every predicate that decides a drop's status or
   * the wrap structure of its polygon is checked against an error bound; a drop that comes close is evaluated in float64)
   * and the environment-map sums under the polygon.  They only feed the drop's colour constants, which only scale
   * rainy_image (contract: +-1 LSB; the mask and the drop statuses never see the difference). */
  RR_OPT_FOV_F32 = 10,
  RR_OPT_FOV_DDA = 12,              /* tuning: the float colour branch evaluates a drop's field-of-view polygon and its row spans with one
                                     * thread per drop (two cursors down the polygon's sides; wrapping polygons and float64 decisions
                                     * through a list to the edge-parallel kernel) -- 1 (default): an exact division per cursor and row;
                                     * 2 (r05): incremental cursors over per-edge records (a quarter of the instructions per row, no
                                     * faster: profiles/r05_ab_log.md); 0: the edge-parallel kernel for every drop.  The spans are the
                                     * same: identical results. */
  RR_OPT_COMPOSITE_WAVES = 11,      /* retired: only 0 is accepted */
  RR_OPT_PIPELINE_F32 = 13,         /* 1 (default): rr_pipeline_* hand the fog layer and the xyY map from the pre-pass to the hot path
                                     * as float32 unless pre_out asks for float64 copies (see rr_pipeline_frames); 0: float64 */
  RR_OPT_WILD_PIXELS = 14,          /* 1: rainy_bg may hold values outside [0, 1] (a third party's array; the fog pre-pass ends with a
                                     * clip, so its output never does).  The reference blends a drop over its whole padded rectangle
                                     * (bad_weather.py:429-446): where the drop image is zero that is np.clip(pixel, 0, 1), a no-op for
                                     * values in [0, 1] -- the library never visits the pad.  With this option the pads are tracked
                                     * (two int32 per pixel, one more kernel) and a pixel some pad reaches before any tile is clipped
                                     * first: the reference's result for any input.  Default 0.  Not with rr_ext_tile. */
  RR_OPT_PNG_DEFLATE = 15,          /* 1: rr_frame_out.rainy_png / mask_png are entropy-coded on the device.  The buffer (same size) then
                                     * starts with 16 bytes {'R','R','Z','1', uint32 length L, 0, 0} followed by the L bytes of the file's
                                     * zlib stream (one dynamic-Huffman deflate block per 32 KB of scanlines; any inflate reads it):
                                     * the IDAT payload as it is.  A file whose stream would not fit its buffer (incompressible pixels)
                                     * keeps its scanlines (first byte = a filter type, never 'R').  rr_png_write_scanlines /
                                     * rr_io_write_frames take either form.  Default 0 (scanlines). */
  RR_OPT_COMPOSITE_U16 = 16,        /* retired: only 1 is accepted */
  RR_OPT_BLUR_DMA = 17,             /* retired: only 1 is accepted */
  RR_OPT_FOV_FILL_RULE = 18,        /* which restatement of cv2.fillConvexPoly (bad_weather.py:388) decides the texels of a drop's field of
                                     * view: 1 (default) OpenCV 3.2's own algorithm -- Bresenham outline + 16.16 edge walkers, in closed
                                     * form per edge and row (csrc/rr_device.h fov_rowspan_cv) -- for the closed polygons it is defined
                                     * for, on the fast colour path as well as the general one (polygons it is not defined for, the
                                     * wrapping ones above all, keep the span rule); 0 the row-span rule (nearest x of every edge on the
                                     * row, min / max).  Colour only: a drop's colour constants move by <= 0.3 %, rainy_image by <= 1 LSB
                                     * on 1.4 % of its values (README, profiles/r05_fill_rule_study.txt); mask and statuses are the same. */
  RR_OPT_BIN_ROWS = 19,             /* retired: only 1 is accepted */
  RR_OPT_COLOUR_STREAM = 21,        /* tuning (r05): two chains of the step that only meet in k_colour run on two streams of the library.
                                     * 1 (default): the FOV chain (polygons, spans, sums over the environment map) on the second stream
                                     * beside plan .. tiles .. blur; 0: one in-order stream (r04).  (2 was the other split -- plan .. lists
                                     * and k_colour on the second stream -- measured slower in r05 and removed in r06: it runs as 1.)
                                     * Same results (with 1 a drop without a FOV polygon gets its raw tile rendered for nothing -- it is
                                     * still not blended and keeps its status -- and such tiles take arena space: the arena grows to the
                                     * batches' own demand, RR_E_ARENA, so this only shows as a slightly larger arena). */
  RR_OPT_TILE_ROWS = 22,            /* tuning (r06): 1, 2 rotate + flip + INTER_AREA tiles (Medium / Small drops, generator.py:163-170)
                                     * are rendered by k_tile_rows -- the batch's tiles in one list bucketed by texture, a wave per tile,
                                     * a lane per canvas row, horizontal folds in registers; 0: k_tile (a workgroup per tile).  2 (default):
                                     * the Big drops' bicubic warps (generator.py:126-132) ride in the same list, their zero-bordered texture
                                     * resident in LDS, a lane per pixel; 1: those stay with k_tile_big (a thread per pixel of a frame's
                                     * concatenated tiles, texels from global memory).  Same bits. */
  RR_OPT_ROWS_SHARES = 23,          /* tuning (r06): k_tile_rows' workgroups take the batch's tile list in shares of equal estimated cost off a
                                     * device-wide counter; this many shares per workgroup (1 .. 8, default 2): more shares even out the
                                     * workgroups, fewer leave less waiting at a share's end */
  RR_OPT_FIELD_CHUNKS = 24,         /* tuning: workgroups that share one frame's slots in the field model's particle kernel
                                     * (rr_set_particle_model): 0 (default: the library sizes it so that a small batch still fills
                                     * the chip, one per frame for large batches) or 1 .. 64.  Same bits. */
  RR_OPT_FOV_ORDER = 25,            /* tuning: which drops share a wave of the thread-per-drop polygon walk (k_fov_dda).  A wave runs the
                                     * walk's vertex path on every row on which one of its 64 polygons has a vertex, so 1 (default)
                                     * sorts a frame's drops by (distance from the camera in 0.25 m buckets, top row of the polygon)
                                     * before the walk: neighbours on the map, of like size, share vertex rows.  0: table order, through
                                     * the same kernels (every sort key is 0).  Same bits.  (bench.py --sweep restores the options it does
                                     * not know to 0: after a sweep this one is off until it is set again.) */
  RR_OPT_STREAK_LEAN = 26,          /* 0 (default): the reference's rule -- a rotated (Medium / Small) tile is flipped when its streak
                                     * ENDS in the right half of the image (generator.py:165) and its corner is the streak's START
                                     * (generator.py:171): right for streaks that radiate from the image centre only.  1: both come
                                     * from the streak's own end points: flip = x1 > x0 (the tile then leans like the streak,
                                     * whether it runs down or up the image: rr_device.h plan_drop) and the corner
                                     * (min(x0, x1), min(y0, y1)), so that a uniform slant (rr_set_particle_wind) leans the same way
                                     * all over the image.  Tile size, rotation terms, resize route, Big drops, external tiles,
                                     * defocus, crop, 'white' and the raw-tile key (it carries the flip) keep their values.  Every
                                     * entry point, XML drop tables and angular noise included: the record's end points decide. */
  RR_OPT_COMPOSITE_BATCH = 20       /* retired: only 1 is accepted */
};
int rr_set_option(rr_ctx* ctx, int32_t option, int32_t value);

/* Asynchronous form of rr_pipeline_frames (pre may be NULL: then it is the asynchronous rr_render_frames): up to
 * RR_PIPE_SLOTS batches in flight.  The upload of one batch, the kernels of another and the download of a third
 * overlap (three streams inside the library).  Buffers must stay valid and untouched until rr_pipeline_wait(slot)
 * returns; buffers from rr_host_alloc (pinned) move at PCIe rate, pageable ones serialise the copies.
 * rr_pipeline_wait returns RR_E_ARENA when the tile arena had to grow: submit that batch again. */
#define RR_PIPE_SLOTS 3
int rr_pipeline_submit(rr_ctx* ctx, int32_t slot, int32_t n, const rr_prepass_in* pre, const rr_frame_in* in,
                       const rr_frame_out* out, const rr_prepass_out* pre_out);
int rr_pipeline_wait(rr_ctx* ctx, int32_t slot);
/* Page-locked host memory (hipHostMalloc) for the buffers of the host-pointer entry points.  A block belongs to its
 * context: rr_destroy releases whatever rr_host_free has not. */
int rr_host_alloc(rr_ctx* ctx, void** out, int64_t bytes);
/* rr_host_alloc / rr_host_free may run on another thread than the context's calls, so their failures are not reported
 * through rr_last_error(): this returns the message of the last failed rr_host_alloc ("" after a successful one); the
 * pointer stays valid until the next rr_host_alloc on the context. */
const char* rr_host_last_error(rr_ctx* ctx);
int rr_host_free(rr_ctx* ctx, void* p);

/* Work-list sizes of frame `frame` of the last batch (after completion): out[0] drops whose raw tile went
 * through the rotate+resize kernels (k_tile_rows + k_tile), [1] through the generic kernel, [2] fused-blur work items, [3] slow-blur
 * drops, [4] small-blur drops, [5] Big drops (bicubic warp: k_tile_big and, with RR_OPT_TILE_ROWS 2, k_tile_rows), [6] the
 * pixels of those Big tiles (sum of tw x th), [7] drops that re-used another drop's bit-identical raw tile (k_dedup). */
int rr_batch_counts(rr_ctx* ctx, int32_t frame, int32_t out[8]);

/* Per-kernel timing with HIP events on the launch stream (off by default). */
int rr_profile_enable(rr_ctx* ctx, int32_t on);
int rr_profile_reset(rr_ctx* ctx);
int rr_profile_read(rr_ctx* ctx, rr_kernel_stat* out, int32_t cap);   /* returns #entries or <0 */

/* What the context holds right now: out[0] device blocks and [1] their bytes, [2] pinned host blocks and [3] their bytes.
 * Every allocation of the library on behalf of the context is counted; the caller's own rr_host_alloc blocks are not.  Reads
 * host-side records only (no device call, no synchronisation). */
int rr_debug_mem(rr_ctx* ctx, int64_t out[4]);

/* Host-only helper (no device, no ctx): the random draws of one frame's drop loop, bit-identical to
 * numpy's legacy global RandomState after np.random.seed(seed) (generator.py:318): per drop one
 * randint(tex_lo[k], tex_lo[k]+10) (bad_weather.py:252-264) and, for non-Big drops, one
 * normal(0, noise_std) (generator.py:136; noise[k] is the raw deviate, 0 for Big drops).  Lets a
 * driver prepare frames on worker threads instead of the process-global generator. */
int rr_host_drop_draws(uint32_t seed, int32_t n, const int32_t* tex_lo, const uint8_t* is_big, double noise_std,
                       int32_t* tex_index, double* noise);

/* Host-only (no device, no ctx, no Python interpreter lock): one frame's drop table from the column store of its
 * simulated frame.  rr_host_frame_draws applies the frame filter (common/generator.py:413-420), picks the texture block
 * (bad_weather.py:250-265; ratio_db = DBManager.ratio, >= 4 entries) and makes the frame's draws in the reference's order;
 * returns the number of kept streaks (<= t->n; keep / tex_index / noise need that capacity), noise = raw deviate * 1.
 * rr_host_assemble_drops writes the rr_drop records once the caller has evaluated cos / sin of the rotation. */
typedef struct {
  int64_t n;
  const double *wps, *wpe;        /* [n][3] world_position_start / _end */
  const int64_t *ips, *ipe;       /* [n][2] image_position_start / _end (integers) */
  const double *iw1, *iw2, *ratio;
  const int64_t *max_width, *length;
  const int32_t* type;            /* DropType */
} rr_streak_table;
int64_t rr_host_frame_draws(const rr_streak_table* t, int32_t W, int32_t H, const double* ratio_db, int32_t n_ratio,
                            uint32_t seed, double noise_std, int64_t* keep, int32_t* tex_index, double* noise);
int rr_host_assemble_drops(const rr_streak_table* t, int64_t n_keep, const int64_t* keep, const int32_t* tex_index,
                           const double* rot_cos, const double* rot_sin, rr_drop* out);
int rr_sizeof_streak_table(void);
/* A whole batch of drop tables in one call, for runs without angular noise (the reference's default): frame k = the filter,
 * draws and records of rr_host_frame_draws + rr_host_assemble_drops on tables[k] with seed seeds[k].  Without noise the
 * rotation terms belong to the table ENTRY: rot_cos[k] / rot_sin[k] hold them for every entry of tables[k] (the caller's
 * numpy evaluates them once per simulated frame; frames that share a table pass the same arrays).  Frame k's records go to
 * out + k * out_stride (records), at most cap of them; counts[k] = the number of kept streaks (it may exceed cap: size up
 * and call again) or a negative RR_E* code.  Runs on `threads` worker threads inside the library (<= 0: up to 16). */
int rr_host_pack_frames(int32_t n, const rr_streak_table* const* tables, const double* const* rot_cos, const double* const* rot_sin,
                        int32_t W, int32_t H, const double* ratio_db, int32_t n_ratio, const uint32_t* seeds, rr_drop* out,
                        int64_t out_stride, int64_t cap, int32_t threads, int64_t* counts);

/* Host-only (no device, no ctx): the particles XML of the rain simulator -> flat records, replacing the reference's
 * pure-Python walk (common/bad_weather.py:192-211).  Raw attribute values only; the derived fields (render scale, y flip,
 * z sign, widths, ratio, rounding, the pid dictionary; bad_weather.py:208-241) stay with the caller.  Counts are always
 * returned; records beyond the capacities are not stored (call again with larger arrays). */
typedef struct {
  int64_t id, t, d, rs;           /* frame attributes id, t (exposure), d (start time), rs (count) */
  int64_t first_drop, n_drops;    /* its drops are records [first_drop, first_drop + n_drops) */
} rr_particle_frame;
typedef struct {
  int64_t pid;
  double wp1[3], wp2[3], wd1, wd2, ip1[2], ip2[2], iw1, iw2;
} rr_particle;                    /* 120 bytes */
int rr_host_parse_particles(const char* path, rr_particle_frame* frames, int64_t cap_frames, rr_particle* drops,
                            int64_t cap_drops, int64_t* n_frames, int64_t* n_drops);
int rr_sizeof_particle(void);
int rr_sizeof_particle_frame(void);

/* Host-only PNG codec for the driver's I/O threads (rr_png.cpp; zlib inside; no interpreter lock when called through
 * ctypes).  Readers: non-interlaced gray / RGB / palette / RGBA files, else RR_E_UNSUPPORTED (use a general decoder).
 *   rr_png_read_bgr8    what cv2.imread(path) returns for an 8-bit file: H*W*3 bytes, B G R      (generator.py:352)
 *   rr_png_read_gray16  cv2.imread(path, IMREAD_UNCHANGED) of a 16-bit single-channel file       (generator.py:360-365)
 *   rr_png_write_scanlines  an RGBA file from H rows of 1 + 4*W filtered bytes (rr_frame_out.rainy_png / mask_png);
 *                           zlib level 0..9, strategy 0 default / 1 Z_RLE / 2 Z_HUFFMAN_ONLY / 3 the library's own
 *                           run-length + dynamic-Huffman deflate (level ignored; an ordinary zlib stream, about the size
 *                           of Z_RLE's at a fifth of the CPU time); rows that begin with 'R','R','Z','1' are a stream the
 *                           device made (RR_OPT_PNG_DEFLATE) and go out as the IDAT payload as they are
 *   rr_deflate_fast     that encoder on n arbitrary bytes -> zlib stream in out (capacity >= rr_deflate_bound(n));
 *                       returns the stream's length or a negative RR_E* code */
int rr_png_info(const char* path, int32_t* w, int32_t* h, int32_t* channels, int32_t* bit_depth);
int rr_png_read_bgr8(const char* path, uint8_t* out, int32_t H, int32_t W);
int rr_png_read_gray16(const char* path, uint16_t* out, int32_t H, int32_t W);
int rr_png_write_scanlines(const char* path, const uint8_t* rows, int32_t W, int32_t H, int32_t level, int32_t strategy);
int64_t rr_deflate_bound(int64_t n);
int64_t rr_deflate_fast(const uint8_t* in, int64_t n, uint8_t* out, int64_t cap);
/* The readers' own inflate (64-bit bit buffer, 12-bit table look-ups that yield two literals where both codes fit, 8-byte
 * match copies; 2-3 times zlib's speed on image scanlines) on a complete
 * zlib stream of known decoded size: 1 = out holds the data (Adler-32 verified), 0 = not vouched for (the readers then
 * hand the stream to zlib), < 0 = bad argument. */
int rr_inflate_fast(const uint8_t* in, int64_t n, uint8_t* out, int64_t out_len);
/* Batch forms for the driver, on `threads` worker threads inside the library (<= 0: up to 16); one call per pipeline batch
 * instead of one interpreter call per frame and file.  The calls return RR_OK unless an argument is bad; status[k] holds
 * frame k's own result (RR_OK, RR_E_ARG: size mismatch / unreadable path, RR_E_UNSUPPORTED, RR_E_PARSE).
 *   rr_io_read_frames   frame k: rr_png_read_bgr8(image_paths[k]) into bg_u8 + k * bg_stride (bytes) and, when depth_paths
 *                       is given, the 16-bit depth file as float32 metres (value / 256, generator.py:360-365) into
 *                       depth_f32 + k * depth_stride (bytes); both files must be H x W
 *   rr_io_write_frames  frame k: rr_png_write_scanlines(strategy 3) of rows_image + k * rows_stride to image_paths[k] and of
 *                       rows_mask + k * rows_stride to mask_paths[k] (either path array may be NULL) */
int rr_io_read_frames(int32_t n, const char* const* image_paths, const char* const* depth_paths, int32_t H, int32_t W,
                      uint8_t* bg_u8, int64_t bg_stride, float* depth_f32, int64_t depth_stride, int32_t threads, int32_t* status);
/*   rr_io_read_frames_u16  the same with the depth file's uint16 samples as they are (rr_prepass_in.depth_f64 = RR_DEPTH_U16) into
 *                       depth_u16 + k * depth_stride (bytes): no conversion pass on the host, half the bytes over PCIe */
/*   rr_io_read_frames_rows  both files of a frame INFLATED ONLY: image_rows + k * image_stride receives H rows of 1 + 3*W bytes (filter
 *                       type + filtered R G B bytes) of the 8-bit RGB image, depth_rows + k * depth_stride H rows of 1 + 2*W
 *                       bytes of the 16-bit gray depth file -- what rr_prepass_in takes with RR_IN_BG_PNG_ROWS /
 *                       RR_DEPTH_PNG_ROWS: the scanline filters are reversed on the device (csrc/rr_pngrows.h), 40 % of the
 *                       host's decode time.  A file of another kind that the readers above accept is decoded on the host
 *                       and handed over as rows of filter type 0. */
int rr_io_read_frames_rows(int32_t n, const char* const* image_paths, const char* const* depth_paths, int32_t H, int32_t W,
                           uint8_t* image_rows, int64_t image_stride, uint8_t* depth_rows, int64_t depth_stride, int32_t threads,
                           int32_t* status);
/*   rr_io_read_frames_rows_sized  the same with depth files of their own size depth_H x depth_W (rows of 1 + 2 depth_W bytes): the
 *                       loader of a context armed with rr_set_input_resize, which resizes both on the device */
int rr_io_read_frames_rows_sized(int32_t n, const char* const* image_paths, const char* const* depth_paths, int32_t H, int32_t W,
                                 int32_t depth_H, int32_t depth_W, uint8_t* image_rows, int64_t image_stride, uint8_t* depth_rows,
                                 int64_t depth_stride, int32_t threads, int32_t* status);
int rr_io_read_frames_u16(int32_t n, const char* const* image_paths, const char* const* depth_paths, int32_t H, int32_t W,
                          uint8_t* bg_u8, int64_t bg_stride, uint16_t* depth_u16, int64_t depth_stride, int32_t threads, int32_t* status);
/*   rr_io_read_frames_scaled  the same for a render scale other than 1 (generator.py:352-381, the Cityscapes plug-in's
 *                       default): image / 255 resized (cv2.resize, INTER_LINEAR) to W x H = file size // render_scale as
 *                       float64 into bg_f64 + k * bg_stride (bytes), the depth map resized to
 *                       (its size * depth_scale) // render_scale when that differs from its own size; both must come out
 *                       H x W (RR_E_ARG otherwise: the reference crops the image then -- the caller's general loader) */
int rr_io_read_frames_scaled(int32_t n, const char* const* image_paths, const char* const* depth_paths, int32_t H, int32_t W,
                             int32_t render_scale, int32_t depth_scale, double* bg_f64, int64_t bg_stride, float* depth_f32,
                             int64_t depth_stride, int32_t threads, int32_t* status);
int rr_io_write_frames(int32_t n, const char* const* image_paths, const char* const* mask_paths, const uint8_t* rows_image,
                       const uint8_t* rows_mask, int64_t rows_stride, int32_t W, int32_t H, int32_t threads, int32_t* status);
/*   rr_io_write_frames_text  one file kind per call: frame k's rows + k * rows_stride to paths[k] (a NULL path is skipped), with
 *                       one tEXt chunk `keyword` NUL texts[k] between IHDR and IDAT -- the layer file's `rain-shift`.  texts == NULL
 *                       (or texts[k] == NULL) writes no chunk: the file is then byte for byte rr_io_write_frames'.  The library
 *                       embeds the bytes as they are; the caller formats them.  RR_E_ARG: with texts, a keyword that is not 1 to
 *                       79 bytes of printable Latin-1 (32..126, 161..255) without leading, trailing or doubled spaces. */
int rr_io_write_frames_text(int32_t n, const char* const* paths, const uint8_t* rows, int64_t rows_stride, int32_t W, int32_t H,
                            const char* keyword, const char* const* texts, int32_t threads, int32_t* status);
/* The codec's checksums: zlib's adler32(adler, p, n) and crc32(crc, p, n) (same values, same chaining; start from 1 and 0),
 * computed with SSSE3 / carry-less multiplication where the CPU has them (zlib's own loops otherwise). */
uint32_t rr_adler32(uint32_t adler, const uint8_t* p, int64_t n);
uint32_t rr_crc32(uint32_t crc, const uint8_t* p, int64_t n);

/* Baseline JPEG input frames (csrc/rr_jpeg.h): the host parses the file and decodes its Huffman stream, the
 * device dequantises, runs the 8x8 inverse DCT, upsamples chroma and converts to B G R (k_jpeg_idct, k_jpeg_bgr).  Between the
 * two travels a frame's COEFFICIENT RECORD: an rr_jpeg_header, then int16 coefficients -- not dequantised, in natural
 * (de-zigzagged) order, 64 per block, a component's blocks in raster order over its plane padded to whole MCUs, Y then Cb then Cr.
 * Taken: SOF0, 8-bit samples, 8-bit tables, ONE interleaved scan of three components in 4:4:4, 4:2:2 (2x1,1x1,1x1) or 4:2:0
 * (2x2,1x1,1x1) -- W >= 3 where chroma is subsampled horizontally -- or of one component; restart intervals.  Anything else
 * (progressive, extended, arithmetic coding, 12 bits, other samplings, four components, several scans, 16-bit tables) is
 * RR_E_UNSUPPORTED; truncated or inconsistent data RR_E_PARSE; an unreadable path or a size that is not the expected one
 * RR_E_ARG.  rr_jpeg_last_error() gives the calling thread's last refusal in a line ("" after a success).
 *   rr_jpeg_info          0 only for a file the reader takes; components 1 / 3, sampling an RR_JPEG_* code
 *   rr_jpeg_record_bytes  a record's size for that frame size and sampling (< 0: bad arguments)
 *   rr_jpeg_read_record   the record of `path` into dst (dst_bytes >= rr_jpeg_record_bytes of the file)
 *   rr_jpeg_read_bgr8     the whole decode on the host through the same arithmetic: H*W*3 bytes, B G R -- byte for byte what
 *                         the device makes of the record
 *   rr_io_read_frames_jpeg  the batch form (see rr_io_read_frames_rows): frame k's record into records + k * record_stride,
 *                         its 16-bit gray depth PNG as H rows of 1 + 2*W filtered bytes into depth_rows + k * depth_stride
 *                         (RR_DEPTH_PNG_ROWS); status[k] as in the other batch readers
 * rr_prepass_in.in_types = RR_IN_BG_JPEG (host-pointer entry points only: rr_pipeline_submit / rr_pipeline_frames /
 * rr_prepass_frames): `bg` points at the frame's record.  For every frame of a batch or for none, not with bg_u8 or
 * RR_PRE_ENV_ONLY, not while rr_set_input_resize is armed; every record's W, H the batch's and its sampling the first frame's
 * (RR_E_ARG with nothing enqueued otherwise).  depth_f64 may be any kind. */
#define RR_JPEG_MAGIC 0x314a5252u /* "RRJ1" */
enum { RR_JPEG_444 = 0, RR_JPEG_422 = 1, RR_JPEG_420 = 2, RR_JPEG_GREY = 3 };
typedef struct {
  uint32_t magic;                 /* RR_JPEG_MAGIC */
  int32_t W, H;
  int32_t sampling;               /* RR_JPEG_* */
  int32_t components;             /* 1 or 3 */
  int32_t reserved[3];            /* 0 */
  uint16_t q[3][64];              /* quantisation table of component c, natural order (unused components: 0) */
} rr_jpeg_header;                 /* 416 bytes */
int rr_jpeg_info(const char* path, int32_t* W, int32_t* H, int32_t* components, int32_t* sampling);
int64_t rr_jpeg_record_bytes(int32_t W, int32_t H, int32_t sampling);
int rr_jpeg_read_record(const char* path, void* dst, int64_t dst_bytes);
int rr_jpeg_read_bgr8(const char* path, uint8_t* dst, int32_t H, int32_t W);
int rr_io_read_frames_jpeg(int32_t n, const char* const* image_paths, const char* const* depth_paths, int32_t H, int32_t W,
                           uint8_t* records, int64_t record_stride, uint8_t* depth_rows, int64_t depth_stride, int32_t threads,
                           int32_t* status);
const char* rr_jpeg_last_error(void);
int rr_sizeof_jpeg_header(void);

/* sizes, for binding self-checks */
int rr_sizeof_drop(void);
int rr_sizeof_camera(void);
int rr_sizeof_frame_in(void);
int rr_sizeof_frame_out(void);
int rr_sizeof_prepass_in(void);
int rr_sizeof_prepass_out(void);
int rr_sizeof_prepass_kernels(void);

#ifdef __cplusplus
}
#endif
#endif /* RAINHIP_H */
