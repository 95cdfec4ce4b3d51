/*
 * cetpick_hip.h - C-ABI of the MI355X (gfx950) hot path for nextpyp/cet_pick (MiLoPYP).
 *
 * The reference is pure Python on PyTorch and has no FFI of its own; its
 * boundary for this path is the Python API.  The Python mirror in cet_pick_amd/ keeps that API
 * (same names / arguments) and reaches the device only through the entry points declared here,
 * via ctypes.  Each entry point cites the reference code it replaces (paths relative to the
 * reference root, cet_pick/...).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors); the caller keeps it
 *    alive until the stream has passed the call;
 *  - every function enqueues work on `stream` and returns without synchronising the device;
 *  - return 0 = ok, negative = argument error (MI_E_*), positive = hipError_t;
 *  - no function allocates device memory: scratch comes from the caller, sized by the matching
 *    *_workspace_bytes() query;  launches are hipGraph-capturable;
 *  - volumes are (D,H,W) row-major fp32 ("Z,H,W" in the reference's in-memory order);
 *    activations of the training path are channels-last (N,D,H,W,C) fp32.
 */
#ifndef CETPICK_HIP_H
#define CETPICK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mi_stream_t; /* hipStream_t */

#define MI_OK 0
#define MI_E_ARG (-1)       /* bad shape / null pointer / unsupported window */
#define MI_E_WORKSPACE (-2) /* workspace too small */
#define MI_E_UNSUPPORTED (-3)

/* Library identity: returns the ABI version (bumped on any signature change). */
int mi_abi_version(void);
/* measurement aid: nodes of a captured hipGraph (hipGraph_t) by type: counts[4] = kernel, memcpy, memset, other */
int mi_graph_node_counts(void* graph, int* counts);
/* measurement aid: a one-thread launch that writes the 100 MHz wall clock into *slot (device uint64) */
int mi_debug_stamp(void* slot, mi_stream_t stream);
/* measurement aid: the kernel family the last mi_conv* call of the calling thread dispatched to (tools/bench_conv.py) */
const char* mi_debug_last_conv_kernel(void);
/* test aid: the schedule of the calling thread's last implicit-GEMM launch ("implicit GEMM ..." above), read-only.  Writes up to n of
 * bm, bn, bk, splits actually used, row classes, border (0/1), fold (0/1), wbox (0/1, as the kernel applies it), grid blocks (x),
 * bf16x3 kernel (0/1), stem (0/1) into out, in this order; returns the number of values written */
int mi_debug_last_conv_plan(int* out, int n);
/* gfx target the code objects were built for, e.g. "gfx950". */
const char* mi_build_arch(void);

/* ------------------------------------------------------------------------------------------
 * Inference path
 * ------------------------------------------------------------------------------------------ */

/* models/utils.py:167-169  `_sigmoid`: x <- sigmoid(x) IN PLACE; y <- clamp(x, 1e-4, 1-1e-4).
 * y may alias x. */
int mi_sigmoid_clamp(float* x, float* y, size_t n, mi_stream_t stream);

/* models/decode.py:11-33 `_nms_xy` (1,k,k) / `_nms_z` (k,1,1) / `_nms` (3,k,k) and
 * utils/image.py:97-105 `_nms` (k,k,k):  out = heat * (max_pool3d(heat, (kd,kh,kh), stride 1,
 * pad (k-1)/2, -inf padding) == heat).   kd, kh odd, in {1,3,5,7}.  out must not alias heat. */
int mi_nms3d(const float* heat, float* out, int D, int H, int W, int kd, int kh,
             mi_stream_t stream);

/* Fused detector decode = `_sigmoid` + `tomo_decode` (models/decode.py:123-155, reg=None) for one
 * (1,1,D,H,W) volume:
 *   heat_out = clamp(sigmoid(logits))            (if apply_sigmoid; heat_out may be NULL)
 *   nms      = `_nms` window (3,k,k)             (fiber != 0: `_nms_xy` (1,k,k) then `_nms_z` (k,1,1))
 *   top-K of nms by (score desc, flat index asc) -> dets[K][5] = {x+.25, y+.25, z, score, score}
 * x,y,z follow `_convert_1d_to_3d` (decode.py:35-41).  Rows past the number of positive local
 * maxima are {0.25,0.25,0,0,0} (torch.topk leaves their order unspecified).
 * n_valid_out (device int32, may be NULL) receives min(K, #positive maxima).
 * logits must not alias heat_out.
 * apply_sigmoid: bit 0 = apply `_sigmoid`; bit 1 = "the workspace header is clean": the caller zeroed it once with
 * mi_decode_workspace_init and has since used the workspace only through calls that passed this bit - such a call
 * skips its own clearing pass and leaves the header clean again (one launch less per decode).  Without bit 1 the
 * workspace needs no initialisation. */
size_t mi_decode_workspace_bytes(int D, int H, int W, int K);
int mi_decode_workspace_init(void* workspace, size_t workspace_bytes, mi_stream_t stream);
int mi_sigmoid_nms_topk(const float* logits, float* heat_out, int D, int H, int W, int k,
                        int fiber, int apply_sigmoid, int K, float* dets, int32_t* n_valid_out,
                        void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* scipy.ndimage.gaussian_filter as called by utils/image.py:152-156 and utils/loader.py:102
 * (mode='reflect', truncate=4 -> radius=int(4*sigma+.5)), separable, fp32 storage,
 * fp32 accumulation.  `tmp` is a scratch volume of D*H*W floats; out may alias in. */
int mi_gauss3d_sep(const float* in, float* out, float* tmp, int D, int H, int W, float sigma,
                   mi_stream_t stream);

/* Per-slice 2-D variant (axes 1 and 2 only): `gaussian_filter(sli, sigma)` in the tilt-series branch of
 * utils/loader.py:94-96. */
int mi_gauss2d_slices(const float* in, float* out, float* tmp, int D, int H, int W, float sigma,
                      mi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Tomogram loading: utils/loader.py `load_rec` :27-88, `quantize` :16-25,
 * `preprocess` :90-121.  Values are evaluated in fp64 registers and stored as fp32.
 * ------------------------------------------------------------------------------------------ */
enum { MI_ORDER_XYZ = 0, MI_ORDER_XZY = 1, MI_ORDER_YXZ = 2, MI_ORDER_ZXY = 3 };   /* `--order` */

/* Axis reorder of an MRC data block `src` of shape (d0,d1,d2) (= mrcfile's .data.shape), element type by
 * MRC mode (0 int8, 1 int16, 2 float32, 6 uint16), into dst (Z',X,Y) fp32 as load_rec does
 * (loader.py:32-36,:62), with `compress`: Z' = ceil(Z/2), slice j = max(slice 2j, slice 2j+1)
 * (loader.py:45-47,:70-71; zxy + compress + odd Z is the reference's IndexError -> MI_E_ARG). */
int mi_rec_reorder(const void* src, int mrc_mode, int d0, int d1, int d2, int order, int compress,
                   float* dst, mi_stream_t stream);
/* stats[s] = {mean, std (ddof 0), min, max} of slice s of x [n_slices][slice_elems] (n_slices = 1: the whole
 * volume, loader.py:59,:87; per slice: the is_tilt branches :48-49,:97). */
size_t mi_vol_stats_workspace_bytes(long n_slices, long slice_elems);
int mi_vol_stats(const float* x, long n_slices, long slice_elems, double* stats, void* ws, size_t ws_bytes,
                 mi_stream_t stream);
/* y = (x - mean) / std per slice (y may alias x). */
int mi_zscore(const float* x, float* y, long n_slices, long slice_elems, const double* stats,
              mi_stream_t stream);
/* preprocess (loader.py:103-106,:118-120): z-score -> q = round(clip(255 (z - mi)/(ma - mi), 0, 255)) ->
 * (q - min q)/(max q - min q).  flat_zero != 0: a constant slice gives 0 (cv2.normalize, :98,:114) instead
 * of NaN.  y may alias x. */
int mi_zscore_quantize_minmax(const float* x, float* y, long n_slices, long slice_elems, const double* stats,
                              double mi, double ma, int flat_zero, mi_stream_t stream);

/* utils/image.py:138-183 `get_potential_coords_pyramid`: DoG pyramid -> border zero (z: border_z
 * slices each end, x/y: 30, or 60 when H>512 and W>512) -> `_nms_xy`(k) -> max over levels ->
 * cutoff = mean(pos)+0.5*std(pos) -> greedy 3-D NMS (`non_maximum_suppression_3d`, distance d).
 * Outputs (device): scores[max_out] fp32, coords[max_out][3] int32 as (x,y,z), n_out int32,
 * cutoff_out fp32 (may be NULL).  Picks are emitted in greedy order (score descending).
 * heat_out (may be NULL) receives the dense NMS'd DoG map (D*H*W).  Volumes of 2^31 voxels or more are
 * refused (MI_E_UNSUPPORTED); their workspace size is a token 256 bytes. */
size_t mi_dog_pick_workspace_bytes(int D, int H, int W, int n_sigmas);
int mi_dog_pick(const float* rec, int D, int H, int W, const float* sigmas_host, int n_sigmas,
                int k, int border_z, int nms_d, float* heat_out, float* scores, int32_t* coords,
                int32_t* n_out, int max_out, float* cutoff_out, void* workspace,
                size_t workspace_bytes, mi_stream_t stream);

/* models/decode.py:42-79 == utils/image.py:42-79 `non_maximum_suppression_3d` on a dense (D,H,W)
 * volume: voxels with value > threshold are visited in (value desc, flat index desc) order; a
 * visited, unsuppressed voxel is emitted and suppresses every flat offset of the radius
 * scale*d/2 ball (flat offsets, no bounds check - wraps exactly like the reference). */
size_t mi_greedy_nms3d_workspace_bytes(int D, int H, int W);
int mi_greedy_nms3d(const float* vol, int D, int H, int W, float d, float scale, float threshold,
                    float* scores, int32_t* coords, int32_t* n_out, int max_out, void* workspace,
                    size_t workspace_bytes, mi_stream_t stream);


/* Sub-tomogram crops, one per centre (x,y,z int32); window along an axis is
 * [c - s/2, c - s/2 + s) as the reference slices it; out-of-volume voxels repeat the edge.
 *   mode 0: raw crop (n, cz, cy, cx)         datasets/tomo_pre_proj_angle_select_new3d_vol.py:130-138
 *   mode 1: sum over z, min-max -> (n, cy, cx)                                          ...:117-128
 *   mode 2: z-normalised 3-D crop (mean 0, unbiased std 1) -> (n, cz, cy, cx)   (MoCo-3D input, §8d C2)
 *   mode 3: ZNormalization -> RescaleIntensity(-3, 3) -> ZNormalization of the crop -> (n, cz, cy, cx)
 *           (datasets/tomo_pre.py:57-60; the `Crop` of that chain is the window the centre and size describe)
 * flip_x mirrors the crop along x (second contrastive view). */
int mi_crop_normalize(const float* vol, int D, int H, int W, const int32_t* centres_xyz, int n,
                      int cz, int cy, int cx, int mode, int flip_x, float* out, mi_stream_t stream);

/* The same crops for a batch whose bookkeeping already lives on the device (replaces the per-batch host work of the
 * reference's DataLoader path, datasets/particle_pre_3d_vol.py:70-85 under moco_main.py:122-130): crop i of the launch
 * is dataset sample s = order[first + i] (order == NULL: s = first + i); it is cut from tomogram vols[owner[s]]
 * (owner == NULL: vols[0]) around centres_xyz[s] (+ shift_xyz[s] when shift_xyz != NULL).  All arrays are device
 * memory.  Modes 0..2 of mi_crop_normalize. */
typedef struct mi_vol_desc {
    const float* vol;
    int32_t D, H, W, reserved;
} mi_vol_desc;
int mi_crop_normalize_table(const mi_vol_desc* vols, const int32_t* owner, const int32_t* centres_xyz,
                            const int32_t* shift_xyz, const int64_t* order, int64_t first, int n, int cz, int cy,
                            int cx, int mode, int flip_x, float* out, mi_stream_t stream);
/* simsiam_test_hm_3d.py:45-51 on min-max'ed crops: y = (floor(255 x) / 255 - mean) / std  (ToPILImage -> ToTensor ->
 * Normalize; mean / std = the dataset statistics of tomo_pre_proj_angle_select_new3d_vol.py:238-239).  y may alias x. */
int mi_u8_roundtrip_normalize(const float* x, float* y, size_t n, float mean, float std, mi_stream_t stream);

/* The mode-2 (z-normalised) crop of samples first .. first + n - 1 of a table (vols, owner, centres_xyz as for
 * mi_crop_normalize_table) in n_poses of the eight in-plane lattice poses of a box with cy == cx (moco_test_3d.py, DESIGN.md
 * 4.26): out (n, n_poses, cz, cy, cx).  Pose p: the crop turned `p & 3` quarter turns as torch.rot90(crop, p & 3, (-2, -1)),
 * then, with `p & 4`, mirrored as torch.flip(crop, (-1,)).  The source window is read once and the statistics are computed
 * once per sample (mi_crop_normalize's, summed in the order of its kernel for these shapes; zero variance divides by zero as
 * it does there): every pose holds the same values, pose q is bit for bit the rotation / mirror image of pose 0.
 * poses: a HOST array of n_poses distinct values in 0..7.  MI_E_ARG: cy != cx, n_poses outside 1..8, a pose outside 0..7 or
 * repeated.  MI_E_UNSUPPORTED: cx > 64, or a window that does not fit the workgroup's LDS (cz cy (cx | 1) floats <= 136 KiB:
 * 32^3 fits, 64^3 does not).  Nothing is launched on either. */
int mi_crop_znorm_poses(const mi_vol_desc* vols, const int32_t* owner, const int32_t* centres_xyz, int64_t first, int n,
                        int cz, int cy, int cx, const int32_t* poses, int n_poses, float* out, mi_stream_t stream);

/* Pose pooling of embeddings: x (n, P, dim) fp32 -> out (n, dim) = normalize(mean over P of normalize(x[i, p, :])), normalize
 * being F.normalize's x / max(|x|, 1e-12).  P == 1: F.normalize(x, dim=1).  One wave per row of out, every sum in a fixed
 * order: the same input gives the same bytes.  P >= 1, 1 <= dim <= 1024 (MI_E_UNSUPPORTED above). */
int mi_embed_pool(const float* x, long n, int P, int dim, float* out, mi_stream_t stream);

/* Random view augmentation of the `simsiam3d` dataset (datasets/tomo_pre_proj_angle_select_new3d_vol.py:49-89: ToPILImage,
 * RandomHorizontalFlip, RandomVerticalFlip, ColorJitter, RandomResizedCrop(aspect 1), ToTensor, FixedRotation
 * (utils/image.py:195-201), Normalize; datasets/particle_pre_3d_vol.py:70-85: the second view is the crop of one of four
 * neighbouring centres).
 *
 * mi_aug2d_params draws table[t] = the parameter record of sample sample_ids[t] for `view` (0 strong, 1 weak; < 256):
 * 8 x 32 bit
 *     word 0  bit 0 hflip, bit 1 vflip, bit 2 bright_first (brightness acts before contrast); other bits reserved, 0
 *     word 1  brightness factor (float32 bits) ~ U(bright_lo, bright_hi)
 *     word 2  contrast factor   (float32 bits) ~ U(contrast_lo, contrast_hi)
 *     word 3  s = round(bbox * sqrt(u)), u ~ U(area_lo, area_hi): side of the square crop window
 *     word 4, 5  i, j: top row and left column of the window, uniform integers in [0, bbox - s]
 *     word 6  k in 0..3: quarter turns, orientation of torch.rot90(img, k, dims=[1, 2])
 *     word 7  neighbour in 0..3: which neighbouring centre's crop the view is made of
 * hflip, vflip ~ Bernoulli(flip_p); bright_first ~ Bernoulli(0.5); k, neighbour uniform.  The generator is Philox-4x32-10
 * with counter (sample id, epoch, view) and key seed: a record is a pure function of (seed, epoch, sample id, view) and of
 * the ranges - no state, no dependence on the position in sample_ids or on n.
 *
 * mi_aug2d_apply: out[t] (bbox x bbox; out is (n, 1, bbox, bbox)) = the chain on crop sample_ids[t] of `bank`
 * ((n_banks, n_samples, bbox, bbox) fp32 in [0, 1]; n_banks > 1: bank table[t].neighbour, clamped) with table[t]:
 *     g = floor(255 x); flips; brightness / contrast in the drawn order, each the 8-bit blend (uint8)(d + f (g - d)) in
 *     single precision, clipped to [0, 255] (brightness: d = 0; contrast: d = int(mean grey level of the current image +
 *     0.5)); window [i : i + s, j : j + s] resized to bbox x bbox, bilinear with half-pixel centres and taps clamped to
 *     the window, rounded to a grey level; / 255; rot90(k); (x - mean) / std.
 * A record's s, i, j are clamped into the crop; a sample id outside [0, n_samples) gives a NaN image.  Both entries take
 * bbox in 8..128 (MI_E_UNSUPPORTED outside); apply runs one workgroup per sample and needs the table 16-byte aligned. */
int mi_aug2d_params(const int64_t* sample_ids, int64_t n, uint64_t seed, int epoch, int view, int bbox, float flip_p,
                    float bright_lo, float bright_hi, float contrast_lo, float contrast_hi, float area_lo, float area_hi,
                    int32_t* table, mi_stream_t stream);
int mi_aug2d_apply(const float* bank, int64_t n_samples, int n_banks, const int64_t* sample_ids, const int32_t* table,
                   int64_t n, int bbox, float mean, float std, float* out, mi_stream_t stream);

/* Random views of the 2d3d dataset (datasets/tomo_pre_proj_angle_select_new2d3d.py:49-82: ToPILImage, RandomHorizontalFlip,
 * RandomVerticalFlip, RandomRotation [strong chain only], CenterCrop(bbox), ToTensor, CornerErasing (utils/image.py:249-321),
 * FixedRotation, Normalize) on the two-channel image (tilt patch, tomogram patch): one record acts on both channels.
 *
 * mi_aug2d3d_params draws table[v][t] = the record of sample sample_ids[t] for view v (0: `strong` ranges, 1: `weak`); table
 * is (2, n, 16) int32.  A record, 16 x 32 bit:
 *     word 0      bit 0 hflip, bit 1 vflip, bit 2 erase (CornerErasing acts); other bits reserved, 0
 *     word 1      k in 0..3: quarter turns, orientation of torch.rot90(img, k, dims=[1, 2])
 *     word 2, 3   i, j: top row and left column of the erased rectangle (they may lie outside the image)
 *     word 4, 5   h, w: its height and width; drawn whether or not bit 2 is set
 *     word 6      the rotation angle in degrees (float32 bits) = angle_lo + (angle_hi - angle_lo) u, not contracted
 *     word 7      reserved, 0
 *     word 8..13  a0..a5: the rotation as the imaging library's 16.16 fixed-point affine map (below), from word 6 in fp64
 *     word 14, 15 reserved, 0
 * hflip, vflip ~ Bernoulli(flip_p); erase ~ Bernoulli(erase_p); k uniform; with mid = bbox / 2, share ~ U(scale), aspect =
 * exp(U(log ratio)): h = round(sqrt(bbox^2 share aspect)), w = round(sqrt(bbox^2 share / aspect)); i uniform in
 * [0, max(1, mid - h - 6)) or in [mid + 6, max(mid + 7, bbox - h + 6)), a fair coin choosing, j likewise with w.
 * The map of rotate(angle, NEAREST, expand=False, fill 0): t = -radians(angle mod 360), m0 = m4 = round(cos t, 15),
 * m1 = round(sin t, 15), m3 = -m1, c = bbox / 2, m2 = m0 (-c) + m1 (-c) + c, m5 = m3 (-c) + m4 (-c) + c, FIX(v) =
 * floor(65536 v + 0.5): a0, a1, a3, a4 = FIX(m0, m1, m3, m4), a2 = FIX(m2 + m0 / 2 + m1 / 2), a5 = FIX(m5 + m3 / 2 + m4 / 2);
 * output pixel (y, x) is input pixel (row (a5 + a4 y + a3 x) >> 16, column (a2 + a1 y + a0 x) >> 16), 0 outside the image.
 * Angle range (0, 0) gives the identity map (65536, 0, 32768, 0, 65536, 32768): the weak chain.
 * The generator is Philox-4x32-10 with counter (sample id, epoch, view | draw << 8 | 0x2D3D0000) and key seed: a record is a
 * pure function of (seed, epoch, sample id, view) and the ranges, and its stream is disjoint from mi_aug2d_params's.
 * MI_E_ARG for ranges with which CornerErasing could reject its first try (h or w reaching mid at the ends of the ranges:
 * the reference's retry loop and its fallback are not built); MI_E_UNSUPPORTED unless bbox is even and in 8..128.
 *
 * mi_aug2d3d_apply: all four tensors of a batch in one launch.  patches_2d, patches_3d: (n_samples, n_variants, bbox, bbox)
 * fp32 in [0, 1].  View 0 of batch row t is made of variant 0 of sample sample_ids[t] with table_strong[t], view 1 of variant
 * variants[t] with table_weak[t].  out is (4, n, bbox, bbox): view 0 channel 2d, view 0 channel 3d, view 1 channel 2d, view 1
 * channel 3d.  Per output pixel: undo the quarter turn; inside the erased rectangle (clipped to the image) the level is 255;
 * else apply the map - outside the image the level is 0, inside it is floor(255 x) (x clamped to [0, 1]) of the source pixel
 * with the flips undone; out = (level / 255 - mean_c) / std_c.  A sample id outside [0, n_samples) or a variant outside
 * [0, n_variants) gives NaN rows and no read; whatever a record holds, no read leaves the patch.  The tables must be 16-byte
 * aligned. */
typedef struct mi_aug2d3d_ranges {
    float flip_p, angle_lo, angle_hi, erase_p, scale_lo, scale_hi, ratio_lo, ratio_hi;
} mi_aug2d3d_ranges;
int mi_aug2d3d_params(const int64_t* sample_ids, int64_t n, uint64_t seed, int epoch, int bbox,
                      const mi_aug2d3d_ranges* strong, const mi_aug2d3d_ranges* weak, int32_t* table, mi_stream_t stream);
int mi_aug2d3d_apply(const float* patches_2d, const float* patches_3d, int64_t n_samples, int n_variants,
                     const int64_t* sample_ids, const int64_t* variants, const int32_t* table_strong,
                     const int32_t* table_weak, int64_t n, int bbox, float mean_2d, float std_2d, float mean_3d, float std_3d,
                     float* out, mi_stream_t stream);

/* Random 3-D views of the MoCo training (datasets/tomo_pre.py:53-62: RandomBlur(p 0.15), RandomNoise(p 0.5), RandomAffine(
 * degrees (0, 60, 0, 0, 0, 0), p 0.75), Crop(size // 8), ZNormalization, RescaleIntensity(-3, 3), ZNormalization;
 * datasets/particle_pre.py:48-87: a flip, then drop_out / center_out / swap_out of utils/image.py:481-536).  c = `crop` is the
 * served edge (even, 6..32); m = c / 6, S = c + 2 m (S / 8 == m), e = S / 8, q = S / 4.  The source of sample s is the S^3 box
 * of tomogram vols[owner[s]] that starts at centre - S / 2 per axis (so its inner c^3 is the crop mi_crop_normalize cuts
 * around the same centre); a box that leaves the tomogram repeats the edge.
 *
 * mi_aug3d_params draws table[v][t] = the record of sample sample_ids[t] for view `view` + v, v < n_views; table is
 * (n_views, n, 16) int32.  A record, 16 x 32 bit:
 *     word 0       bit 0 blur, bit 1 noise, bit 2 rotation act; bits 4-5 flip (0 none, 1 reverse z, 2 reverse y); bits 8-9
 *                  erasure (0 none, 1 drop_out, 2 center_out, 3 swap_out); other bits reserved, 0
 *     word 1..3    sigma z, y, x of the blur (float32 bits), each lo + (hi - lo) u, not contracted; drawn whether or not bit 0 is set
 *     word 4       sigma of the noise (float32 bits)
 *     word 5       the rotation angle in degrees (float32 bits)
 *     word 6, 7    (float) cos, (float) sin of the angle, from word 5 in fp64: t = (double) degrees * (pi / 180)
 *     word 8..10   z, y, x corner of erasure box 0 (drop_out's box, swap_out's first)
 *     word 11..13  z, y, x corner of erasure box 1 (swap_out's second); per axis distinct from box 0's
 *     word 14, 15  k0, k1: the key of the view's noise (below)
 * Draws: Philox-4x32-10 with key (seed low, seed high) and counter (sample id low, sample id high, epoch,
 * view | j << 8 | 0x3D3D0000), j = 0..4, of which words w0..w3; u(w) = (w >> 8) / 2^24:
 *     j = 0   w0: blur iff u < blur_p; w1..w3: sigma z, y, x        j = 1   w0: noise iff u < noise_p; w1: noise sigma;
 *     w2: rotation iff u < rot_p; w3: angle                          j = 2   w0: flip z iff u < flip_z_below, y iff u >
 *     flip_y_above; w1: drop_out iff u < drop_below, else center_out iff u < centre_below, else swap_out iff u < swap_below;
 *     w2, w3: k0, k1         j = 3   w0..w2: index i0 = mulhi(w, N) of box 0's z, y, x corner in the corner set
 *     j = 4   w0..w2: i = mulhi(w, N - 1), box 1's index i1 = i + (i >= i0)
 * The corner set of an axis is [0, c/2 - 2e) U [c/2 + e, c - e) in ascending order, N entries.  A record is a pure function
 * of (seed, epoch, sample id, view) and the ranges; its counters are disjoint from mi_aug2d_params' and mi_aug2d3d_params'.
 *
 * mi_aug3d_apply: out[v][t] (c^3; out is (n_views, n, c, c, c)) = the chain on the box of sample sample_ids[t] with
 * table[v][t]:
 *     blur:     scipy.ndimage.gaussian_filter(box, (sz, sy, sx)): per axis radius r = int(4 sigma + 0.5) (fp64; at most 4), taps
 *               exp(-k^2 / (2 sigma^2)) normalised, edge mode `reflect` at the box's edges, axes z, y, x in turn; r = 0 leaves the axis
 *     noise:    + sigma_n * N(0, 1) per voxel; the deviate of voxel i = (z S + y) S + x of the box is sqrt(-2 ln u1) cos(2 pi u2)
 *               with u1 = ((w0 >> 8) + 1) / 2^24, u2 = (w1 >> 8) / 2^24 of Philox(counter (i, 0, 0, 0x3D3E0000), key (k0, k1))
 *     rotation: output (z, y, x) = plane z sampled at (a + cos (y - a) - sin (x - a), a + sin (y - a) + cos (x - a)), a =
 *               (S - 1) / 2, bilinear; a coordinate outside [0, S - 1] gives the minimum of the blurred, noised box
 *     crop m per side; ZNormalization (unbiased std), RescaleIntensity(-3, 3), ZNormalization: mode 3 of mi_crop_normalize
 *     flip; erasure: drop_out zeroes the e^3 box 0; center_out zeroes all but y, x in [c/2 - q, c/2 + q); swap_out writes box
 *     1's old content to box 0, then box 0's old content to box 1.
 * A step that does not act leaves the values untouched, so a record with only flip / erasure bits gives the mode-3 crop of
 * the same centre, flipped / erased, bit for bit.  Corners are clamped into [0, c - e]; a sample id outside [0, n_samples)
 * gives a NaN view and no read.  table and workspace must be 16-byte aligned; workspace (mi_aug3d_workspace_bytes) holds the
 * blurred, noised boxes and their minima.  Three launches with mi_aug3d_params; no atomics: bit-reproducible.
 * MI_E_ARG: sigma_hi > 1, thresholds outside [0, 1] or out of order; MI_E_UNSUPPORTED: crop odd, outside 6..32. */
typedef struct mi_aug3d_ranges {
    float blur_p, sigma_lo, sigma_hi, noise_p, noise_lo, noise_hi, rot_p, angle_lo, angle_hi, flip_z_below, flip_y_above,
        drop_below, centre_below, swap_below;
} mi_aug3d_ranges;
int mi_aug3d_params(const int64_t* sample_ids, int64_t n, uint64_t seed, int epoch, int view, int n_views, int crop,
                    const mi_aug3d_ranges* ranges, int32_t* table, mi_stream_t stream);
size_t mi_aug3d_workspace_bytes(int64_t n, int n_views, int crop);
int mi_aug3d_apply(const mi_vol_desc* vols, const int32_t* owner, const int32_t* centres_xyz, int64_t n_samples,
                   const int64_t* sample_ids, const int32_t* table, int64_t n, int n_views, int crop, float* out,
                   void* workspace, size_t workspace_bytes, mi_stream_t stream);

/* Tilt-series patches of the 2d3d exploration mode (datasets/tomo_pre_proj_angle_select_new2d3d.py:91-133
 * `convert_tomo_to_tilt` + `extract_patches`), one per centre.  Centre i = (x, y, z_full) of stack owner[i]
 * (owner == NULL: stack 0).  For every tilt t of that stack, in order:
 *     tx = (int)((x - W/2) cos a_t + ((Zfull - z_full) - Zfull/2) sin a_t + W/2)      (fp64, no contraction, trunc)
 *     ty = y;  the tilt is skipped when tx <= bx || tx >= W - bx || ty <= by || ty >= H - by
 * patch = fp32 sum in tilt order of tilts[t, ty-cy/2 : ty+cy/2, tx-cx/2 : tx+cx/2]; out[i] = (p - min) / (max - min)
 * (cy, cx) and valid[i] = 1, or out[i] = 0 and valid[i] = 0 when no tilt survived or min == max.  cos_sin holds
 * cos a_t for t < T and sin a_t at T + t (host-computed fp64).  A tilt whose window would leave the stack is skipped
 * too (never the case for even crops with bx >= cx/2 - 1, by >= cy/2 - 1).  cx, cy even; n <= (2^32 - 1) / 256 (one
 * 256-thread workgroup per centre; MI_E_UNSUPPORTED above).  All arrays device memory. */
typedef struct mi_tilt_desc {
    const float* tilts;       /* (T, H, W) fp32 */
    const double* cos_sin;    /* (2, T) */
    int32_t T, H, W, Zfull;
} mi_tilt_desc;
int mi_tilt_patches(const mi_tilt_desc* stacks, int n_stacks, const int32_t* owner, const int32_t* centres_xyz, int64_t n,
                    int cy, int cx, double bx, double by, float* out, uint8_t* valid, mi_stream_t stream);

/* Label volume of one tomogram for the detector training on coordinate files (datasets/tomo_moco.py:77-130 `load_data`):
 * hm (D, H, W) fp32 is zeroed, then the (2r+1)^3 fp32 stencil (host-computed: gaussian3D or gaussian3D_discrete of
 * utils/image.py, cast once to fp32) is max-combined at each of the n centres (x, y, z) int32, clipped by box intersection
 * with the volume (`draw_umich_gaussian_3d`; centres outside the volume stamp what of their box is inside).  Stencil values
 * must be >= 0: the max is an unsigned atomic max on the fp32 bits (deterministic).  fill_unlabeled != 0: every exact 0
 * becomes -1 afterwards (the train split, :121-123).  Up to three operations on the stream (zero, scatter, fill).  r <= 64;
 * all arrays device memory. */
int mi_semi_labels(float* hm, int D, int H, int W, const int32_t* centres_xyz, int64_t n, const float* stencil, int r,
                   int fill_unlabeled, mi_stream_t stream);
/* The crop pairs of one training batch of the detector (datasets/particle_moco.py:34-163 at down_ratio 2): crop i of the
 * launch is table entry s = first + i, cut around the downscaled centre (x, y, z) = centres_xyz[s] from tomogram
 * tomos[owner[s]] and its label volume labels[owner[s]] (same depth, half the height and width):
 *     input[i]     = tomo[z-3 : z+3, 2y-32 : 2y+32, 2x-32 : 2x+32]        (n, 6, 64, 64)
 *     input_aug[i] = input[i] mirrored along y (flip_y != 0, flip_ud) or x (flip_lr)
 *     hm[i]        = label[z-3 : z+3, y-16 : y+16, x-16 : x+16]           (n, 1, 6, 32, 32)
 * The host draws windows inside both volumes; an entry whose window is not (or whose owner is out of range) reads nothing and
 * gives zeros.  One 256-thread workgroup per crop; all arrays device memory. */
int mi_semi_pairs(const mi_vol_desc* tomos, const mi_vol_desc* labels, int n_tomos, const int32_t* owner,
                  const int32_t* centres_xyz, int64_t first, int n, int flip_y, float* input, float* input_aug, float* hm,
                  mi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training path: channels-last fp32 activations (N,D,H,W,C),
 * weights [tap][Cin][Cout] with tap = (kd*k + kh)*k + kw.
 * ------------------------------------------------------------------------------------------ */

/* One convolution problem, passed by pointer: input (N, Di, Hi, Wi, Ci) -> Co channels, window (kd, kh, kw), one stride for
 * the three axes, zero padding (pd, ph, pw), dilation (dd, dh, dw) (1 = none; a dilated window needs stride 1 and Ci != 1).
 * Output extent per axis = (in + 2 * pad - dil * (k - 1) - 1) / stride + 1.  Window <= 7 per axis, stride 1 or 2,
 * Ci % 16 == 0 (or Ci == 1), Co % 16 == 0. */
typedef struct mi_conv_geom {
    int N, Di, Hi, Wi, Ci, Co, kd, kh, kw, stride, pd, ph, pw, dd, dh, dw;
} mi_conv_geom;

/* nn.Conv3d / nn.Conv2d (D = 1, kd = 1, pd = 0 on (N,1,H,W,C) activations) / nn.Linear (1x1x1 window, D = H = W = 1), no bias
 * of their own, as implicit GEMM on the matrix cores: f32 operands, f32 accumulation; weights [kd][kh][kw][Cin][Cout].  The
 * environment variable MI_CONV_ARITH selects how the f32
 * products are formed: "bf16x3" (default) - every operand element is cut exactly into three bf16 values and the six
 * products of weight <= 2 are accumulated by v_mfma_f32_32x32x16_bf16 (f32-equivalent: the dropped terms are below one
 * f32 rounding; non-finite inputs give NaN where an f32 multiply would give Inf) - or "f32" - v_mfma_f32_32x32x2_f32,
 * bit-for-bit an fmaf chain.  Replaces models/networks/moco_encoder_3d.py:40-84 (conv3x3x3,
 * BasicBlock), :163-169 (7x7x7 stem, Ci == 1), :183, :189, :198-205 (feature conv, fc, proj), the nn.Conv2d of the 2-D
 * encoder (models/networks/simsiam_model_2d.py:25-28, 473-502, 617-661) and the dilated 3-D head of the detector
 * (kernel (3,3,3), dilation (1,4,4), padding (1,4,4): models/networks/unet_small.py:38-41).
 *   fwd:   y  = act(conv(x, w) + res)                 res may be NULL, relu 0/1.  res_is_bias != 0: res is ONE row of Co
 *          values (a bias; NULL is MI_E_ARG) - the reference's conv -> BatchNorm(eval) -> ReLU triple at inference
 *          (models/networks/unet.py:198-249,319-399) once the caller has folded the BatchNorm's scale into w and its shift into bias
 *   dgrad: dx = (conv_transpose(dy, w) + res) * (mask > 0)     res, mask may be NULL
 *   wgrad: dw = sum over output voxels.  splits_out == NULL: dw is final.  Otherwise the split-K reduction is left to the
 *          caller: *splits_out = 1 -> dw is final; > 1 -> `ws` holds that many slabs of Co*Ci*kd*kh*kw floats (slab s at
 *          ws + s * that many floats) and dw is untouched.  mi_splitk_reduce_batch sums the slabs of n such launches
 *          (outs[i] <- sum of n_slabs[i] slabs at slabs[i], out_elems[i] floats each, a multiple of 4) in one launch per 24
 *          of them: one reduce for the weight gradients of a whole backward pass.  Its pointer / count arrays are HOST
 *          arrays (read during the call).
 * `ws` holds split-K slabs and the weight images of the direct kernels (mi_conv_workspace_bytes covers all three passes; 0 = a
 * geometry the entries refuse); a NULL / short ws silently selects the unsplit schedule (same values up to fp32 summation order). */
size_t mi_conv_workspace_bytes(const mi_conv_geom* g);
int mi_conv_fwd_f32(const float* x, const float* w, float* y, const float* res, int res_is_bias, int relu,
                    const mi_conv_geom* g, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_conv_dgrad_f32(const float* dy, const float* w, float* dx, const float* res, const float* mask,
                      const mi_conv_geom* g, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_conv_wgrad_f32(const float* x, const float* dy, float* dw, const mi_conv_geom* g, void* ws, size_t ws_bytes,
                      int* splits_out, mi_stream_t stream);
int mi_splitk_reduce_batch(const void* const* slabs, void* const* outs, const int* n_slabs, const long* out_elems, int n,
                           mi_stream_t stream);
/* Round 5: nb (2..4) weight gradients of ONE geometry in ONE launch - the weight gradients of a residual stage exist together
 * once loss.backward() (trains/base_trainer.py:497) has left the stage (moco_encoder_3d.py:55-84: layer1's four, layer2's and
 * layer3's three equal convolutions), and a launch's fixed costs are a third of each when they run one by one.  Problem i reads
 * xs[i] / dys[i] and leaves *splits_out slabs in wss[i] (each workspace ws_bytes long; > 1: mi_splitk_reduce_batch sums them into
 * dws[i]) or, *splits_out == 1, the final gradient in dws[i].  The pointer arrays are HOST arrays.  MI_E_UNSUPPORTED: no batched
 * kernel for this geometry / nb (or MI_NO_WGRAD_BATCH=1) - issue nb single calls. */
int mi_conv_wgrad_batch_f32(const float* const* xs, const float* const* dys, float* const* dws, void* const* wss, int nb,
                            const mi_conv_geom* g, size_t ws_bytes, int* splits_out, mi_stream_t stream);

/* nn.Linear (+ bias) followed by training-mode nn.BatchNorm1d (+ ReLU) in one launch (the projection MLP,
 * models/networks/moco_encoder_3d.py:238-255): xlin (M, Co) = x W + bias (kept for the backward), y = act(bn(xlin)),
 * save = mean[Co], invstd[Co]; running statistics and num_batches_tracked (int64) are updated when given.  Arithmetic of
 * mi_linear_fwd_f32 followed by mi_bn_small_fwd.  MI_E_UNSUPPORTED for M > 64 or MI_CONV_ARITH=f32: run those two. */
int mi_linear_bn_fwd_f32(const float* x, const float* w, const float* bias, float* xlin, float* y, int M, int Ci, int Co,
                         const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                         float* running_var, long long* num_batches_tracked, float* save_mean_invstd, int relu,
                         mi_stream_t stream);

/* The SyncBatchNorm form of the same fusion (moco_main.py:65-66 converts the encoders): xlin = x W + bias and this rank's column
 * sums of xlin and xlin^2 (2 Co doubles, as mi_bn_stats) from the product's epilogue; the all-reduce of `sums` and
 * mi_bn_apply_fwd follow.  M <= 64 rows. */
int mi_linear_stats_fwd_f32(const float* x, const float* w, const float* bias, float* xlin, double* sums, int M, int Ci, int Co,
                            mi_stream_t stream);

/* conv1 + the batch statistics of bn1 in one pass (models/networks/moco_encoder_3d.py:170-176, 326-328): the 7^3
 * stride-2 single-channel stem convolution, with sums[0..Co) = column sums of y and sums[Co..2Co) = column sums of y^2
 * (device doubles; what mi_bn_stats(y) would produce) taken from the output tiles while they are in registers.
 * MI_E_UNSUPPORTED where the stem kernel does not apply (shape, Co != 64, MI_CONV_ARITH=f32): run mi_conv_fwd_f32 and
 * mi_bn_stats instead.  Workspace: mi_conv3d_stem_stats_workspace_bytes (0 = unsupported shape). */
size_t mi_conv3d_stem_stats_workspace_bytes(int N, int Di, int Hi, int Wi, int Co);
int mi_conv3d_stem_stats_f32(const float* x, const float* w, float* y, int N, int Di, int Hi, int Wi, int Co,
                             double* sums, void* ws, size_t ws_bytes, mi_stream_t stream);

/* nn.Linear (models/networks/moco_encoder_3d.py:183-236: fc and the projection head): y[M][Co] = x[M][Ci] . W + bias with
 * W in kernel layout [Ci][Co]; bias (Co values, may be NULL) is added in the epilogue of the 1x1x1 convolution launch.
 * Workspace as mi_conv_workspace_bytes of the geometry {M, 1, 1, 1, Ci, Co, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1}. */
int mi_linear_fwd_f32(const float* x, const float* w, const float* bias, float* y, int M, int Ci, int Co, void* ws,
                      size_t ws_bytes, mi_stream_t stream);

/* y = act(conv2d(x, w, 7 x 7, stride 2, padding 3) + bias): ONE input channel, 16 output channels, x (N, H, W), w in kernel layout
 * [7][7][1][16], bias[16] or NULL, y (N, Ho, Wo, 16) channels-last with Ho = (H - 1) / 2 + 1 (models/networks/unet_small.py:35: the
 * detector's first layer, with its evaluation-mode BatchNorm folded in by the caller). */
int mi_stem2d_fwd_bias_f32(const float* x, const float* w, const float* bias, float* y, int relu, int N, int H, int W,
                           mi_stream_t stream);
/* Forward convolutions with a short reduction, inference path (round 4; no gradient form - training keeps mi_conv_*_f32): 1 x 1
 * (ntaps 1) or (3, 1, 1) with padding (1, 0, 0) (ntaps 3: `plane` = H * W rows per z-plane, `D` planes per sample) on channels-last rows
 * x (M, Ci) -> y (M, Co) = act(x . W + bias), bias may be NULL.  Ci a multiple of 16, Co of 32.  `img` (mi_smallk_image_bytes(ntaps * Ci, Co)
 * bytes) is written by mi_smallk_prep from the kernel-layout weights [tap][Ci][Co] once per set of weights.  Replaces the implicit GEMM
 * for the detector's 1 x 1 layers and (3, 1, 1) head (models/networks/unet.py:319-399,880-886, unet_small.py:86-97). */
size_t mi_smallk_image_bytes(int K, int Co);
int mi_smallk_prep(const float* w, void* img, int K, int Co, mi_stream_t stream);
int mi_smallk_fwd_f32(const float* x, const void* img, const float* bias, float* y, int relu, long M, int Ci, int Co,
                      int ntaps, long plane, int D, mi_stream_t stream);
/* Round 5: the detector's two heads in ONE pass over the feature volume (unet_small.py:86-97: `proj` = F.normalize(Conv3d(C, 32,
 * (3,1,1), padding (1,0,0))(v)), `hm` = Conv3d(C, K <= 4, (3,1,1))(v)): y_proj (M, 32) normalised in the epilogue, y_hm (M, K) as a
 * by-product of the fragments the product loads (f32 FMAs, as mi_zhead_fwd).  img: mi_smallk_prep(w_proj, img, 3 Ci, 32);
 * w_hm: [3][Ci][K] f32.  M = N D plane rows.  Inference only. */
int mi_smallk_heads_fwd_f32(const float* x, const void* img, float* y_proj, const float* w_hm, float* y_hm, int k_hm, long M, int Ci,
                            long plane, int D, mi_stream_t stream);
/* Patch-resident direct kernels for the 3^3 / stride 1 / padding 1 convolutions of the MoCo-3D encoder's residual layers
 * (models/networks/moco_encoder_3d.py:55-84,170-171), forward and data gradient, bf16x3 arithmetic:
 *   channels 64 : nn.Conv3d(64, 64, 3, 1, 1) on (N, D, 8, 8, 64), D even                  (layer1)
 *   channels 128: nn.Conv3d(128, 128, 3, 1, 1) on (N, 4, 4, 4, 128)                        (layer2)
 * mi_conv_fwd_f32 / mi_conv_dgrad_f32 take them by themselves for such shapes and build
 * the weight image in `ws` on every call (MI_CONV_NO_DIRECT=1 keeps the implicit GEMM).  A caller that knows when the
 * weights change keeps the images instead: mi_conv3d_direct_prep cuts n weight tensors ([tap][Cin][Cout] f32, channels[i]
 * = 64 or 128) into n images of mi_conv3d_direct_wimg_bytes(channels[i]) bytes in one launch per channel count (dgrad[i]
 * != 0: the transposed, tap-flipped image the data gradient needs; the four arrays are HOST arrays), and
 * mi_conv3d_direct_f32 runs
 *   forward  (image with dgrad = 0): out = act(conv(a, w) + res)                       a = x,  relu as given, mask NULL
 *   dgrad    (image with dgrad = 1): out = (conv_transpose(a, w) + res) * (mask > 0)   a = dy, relu 0
 * `ws`: mi_conv3d_direct_workspace_bytes(N, channels) bytes (0 since round 4: both direct kernels are final in one launch; rounds 2-3 kept split-K slabs of the 128-channel kernel there).
 * MI_E_UNSUPPORTED for any other shape (mi_conv3d_direct_usable: 0 / 1 (64 channels) / 2 (128 channels)). */
size_t mi_conv3d_direct_wimg_bytes(int channels);
size_t mi_conv3d_direct_workspace_bytes(int N, int channels);
int mi_conv3d_direct_usable(int N, int Di, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad);
int mi_conv3d_direct_prep(const void* const* w, void* const* img, const int* dgrad, const int* channels, int n,
                          mi_stream_t stream);
int mi_conv3d_direct_f32(const float* a, const void* wimg, float* out, const float* res, const float* mask, int relu,
                         int N, int Di, int Hi, int Wi, int channels, void* ws, size_t ws_bytes, mi_stream_t stream);

/* Round 6: patch-resident direct kernel for the 3 x 3 / stride 1 / padding 1 convolutions of the SimSiam 2-D encoder's BasicBlocks
 * (models/networks/simsiam_model_2d.py:473-502; TomoResClassifier2D.forward :776-819) at --bbox 36 (docs/explore.md:67), forward and
 * data gradient, bf16x3 arithmetic: C -> C channels (64 / 128 / 256) on (N, H, W, C) channels-last planes (csrc/conv_p2d.hip: the batch
 * tiled as ONE flat run of voxels, 128 per workgroup, a zero row between planes).
 *   mi_conv2d_p2d_usable: 1 = a compile-time instance ((W, C) = (36, 64), (18, 128), (9, 256), H >= W: tap offsets are immediates), 2 = the
 *     generic instance (any H, W up to ~64 whose patch fits: run-time geometry - the default --bbox 32 and every other), 0 = neither
 *     (MI_NO_P2D=1: always 0; MI_NO_P2D_GENERIC=1: never 2);  mi_conv2d_p2d_wimg_bytes(C): bytes of one weight image;
 *   mi_conv2d_p2d_prep: n images in one launch from (3, 3, C_i, C_i) kernel-layout weights (dgrad[i] != 0: the transposed,
 *     tap-flipped image of the data gradient; the four arrays are HOST arrays);
 *   mi_conv2d_p2d_f32: out = act(conv(a; image) + res) * (mask > 0); res / mask may be NULL (forward: a = x; dgrad: a = dy, relu 0). */
int mi_conv2d_p2d_usable(int N, int H, int W, int C);
size_t mi_conv2d_p2d_wimg_bytes(int C);
int mi_conv2d_p2d_prep(const void* const* w, void* const* img, const int* dgrad, const int* channels, int n, mi_stream_t stream);
int mi_conv2d_p2d_f32(const float* a, const void* wimg, float* out, const float* res, const float* mask, int relu, int N, int H, int W,
                      int C, mi_stream_t stream);
/* ... and their weight gradient (_workspace_bytes = 0: this shape has none - windows of more than 192 rows, W > ~40): dw (3, 3, C, C) kernel layout = sum over the batch's voxels of x[o + tap] (x) dy[o], written (not
 * accumulated); both operands staged voxel-major and read through the transposing LDS read, X in a padded flat order in which a tap is one
 * row offset; split-K slabs in ws (mi_conv2d_p2d_wgrad_workspace_bytes), added in slab order.  MI_NO_P2D_WGRAD=1: MI_E_UNSUPPORTED. */
size_t mi_conv2d_p2d_wgrad_workspace_bytes(int N, int H, int W, int C);
int mi_conv2d_p2d_wgrad_f32(const float* x, const float* dy, float* dw, int N, int H, int W, int C, void* ws, size_t ws_bytes,
                            mi_stream_t stream);

/* The 2-D encoder's first layer, Conv2d(1, Co, 3, padding=1) (models/networks/simsiam_model_2d.py:634): nine taps of one input channel -
 * HBM-bound f32 FMA chains, not matrix work.  x (N, H, W), w (3, 3, 1, Co) kernel layout, y / dy (N, H, W, Co); Co a multiple of 4, <= 64
 * (else MI_E_UNSUPPORTED).  The weight gradient sums per-block partials in block order (deterministic); ws: _workspace_bytes(Co). */
size_t mi_conv2d_stem3_workspace_bytes(int Co);
int mi_conv2d_stem3_fwd_f32(const float* x, const float* w, float* y, int N, int H, int W, int Co, mi_stream_t stream);
int mi_conv2d_stem3_wgrad_f32(const float* x, const float* dy, float* dw, int N, int H, int W, int Co, void* ws, size_t ws_bytes,
                              mi_stream_t stream);

/* 3^3 / stride 1 / padding 1 convolutions on 2 x 2 x 2 volumes, C -> C channels, C = 128 / 256 / 512 (layer3 and feature_3d
 * of the MoCo-3D encoder, models/networks/moco_encoder_3d.py:55-84,172,178), bf16x3 arithmetic, FINAL IN ONE LAUNCH (round 4:
 * the last of the four reduction quarters of an output tile to arrive sums them - in a fixed order - and applies the epilogue):
 *   dgrad = 0: out = act(conv(a, w) + res)                      a = x (N, 2, 2, 2, C),  w = [27][Cin][Cout] f32, mask NULL
 *   dgrad = 1: out = (conv_transpose(a, w) + res) * (mask > 0)  a = dy, relu 0
 * mi_conv_fwd_f32 / mi_conv_dgrad_f32 take such shapes too (same kernel, partial sums + a reduce launch: their `ws` has no
 * state).  `ws` here: mi_conv3d_cube2_workspace_bytes(N, C) bytes OWNED BY ONE STREAM whose first 16 KiB (arrival counters) are
 * ZERO before the first call; every completed call leaves them zero.  MI_E_UNSUPPORTED for other shapes
 * (mi_conv3d_cube2_usable). */
size_t mi_conv3d_cube2_workspace_bytes(int N, int C);
int mi_conv3d_cube2_usable(int N, int Di, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad);
int mi_conv3d_cube2_f32(const float* a, const float* w, float* out, const float* res, const float* mask, int relu, int dgrad,
                        int N, int C, void* ws, size_t ws_bytes, mi_stream_t stream);

/* Patch-resident direct convolution to 32 output channels, forward / inference (conv_d32.hip): the detector's
 * Conv2d(32|64, 32, 3, padding=1) layers with their BatchNorm folded into weights + bias
 * (models/networks/unet.py:198-249) and the Conv3d(32, 32, 3, padding=(1,4,4), dilation=(1,4,4)) + ReLU of the
 * feature head (models/networks/unet_small.py:52-60).
 *   mi_conv_d32_kind: 1 = 3x3 on every plane (kd = 1, dilation 1, Ci 32 or 64, H and W multiples of 16); 2 = 3x3x3 with
 *     dilation (1,4,4) (Ci 32, H and W multiples of 32, D even); 0 = not taken.  stride 1, padding = dilation * (k - 1) / 2.
 *   mi_conv_d32_prep: w in kernel layout [tap][Ci][32] -> the pre-cut bf16x3 image (mi_conv_d32_image_bytes(Ci, 9 | 27)).
 *   mi_conv_d32_fwd_f32: y = act(conv(x) + bias); x (N, D, H, W, Ci), y (N, D, H, W, 32) channels-last; bias may be NULL. */
int mi_conv_d32_kind(int N, int D, int H, int W, int Ci, int Co, int kd, int kh, int kw, int dd, int dh, int dw);
size_t mi_conv_d32_image_bytes(int Ci, int ntap);
int mi_conv_d32_prep(const float* w, void* img, int Ci, int ntap, mi_stream_t stream);
/* Round 5: the same kernel to 64 output channels (mi_conv_d32_kind returns 3: 2-D 3 x 3, Ci 32 / 64 / 128, H and W multiples of 16 -
 * the 128 x 128 level of the U-Net, unet.py:198-249): image [chunk][tap][column half][plane][lane]; forward through
 * mi_conv_d32_fwd_f32(..., kind = 3) with y (N, D, H, W, 64).  MI_NO_D64=1 keeps the implicit GEMM. */
size_t mi_conv_d64_image_bytes(int Ci, int ntap);
/* Co = 64, 128 or 256 (kind 3 too): one image per 64-column block - img holds (Co / 64) x mi_conv_d64_image_bytes(Ci, 9) bytes -,
 * a workgroup per tile and block; y (N, D, H, W, Co).  MI_NO_D64_WIDE=1 keeps Co > 64 on the implicit GEMM. */
int mi_conv_d64_prep_co(const float* w, void* img, int Ci, int Co, int ntap, mi_stream_t stream);
/* mi_conv_d32_kind = 4: 1 x 1 products (the 2 x 2 transposed convolutions' 4 Co columns, unet.py:251-317, and the last 1 x 1 layer):
 * y = act(x W + bias) per voxel, the tile resident in LDS.  Co = 32 (image: mi_conv_d32_prep(w, img, Ci, 1)) or a multiple of 64
 * up to 512 (mi_conv_d64_prep_co(w, img, Ci, Co, 1)); Ci 32 / 64 / 128 / 256; H % 8 == 0, W % 16 == 0.  MI_NO_D32_1X1=1: off. */
int mi_conv_d32_1x1_fwd_f32(const float* x, const void* wimg, const float* bias, float* y, int relu, int N, int D, int H, int W,
                            int Ci, int Co, mi_stream_t stream);
/* The 2 x 2 / stride-2 transposed convolution of an up-convolution block at inference (unet.py:251-317,319-399) in ONE launch: the
 * 1 x 1 product to 4 Co columns with the pixel shuffle, scale / shift (evaluation-mode BatchNorm, bias folded in) and ReLU in its
 * epilogue, written into out (N, Ho, Wo, cstride)[..., 0:Co] - the first Co channels of the concatenation, whose channels Co.. the
 * caller fills with the encoder feature.  wimg: mi_conv_d64_prep_co(w, img, Ci, 4 Co, 1).  Ci 32 / 64 / 128, Co a multiple of 32 with
 * 64 <= 4 Co <= 512, H % 8 == 0, W % 16 == 0; MI_E_UNSUPPORTED otherwise (then: the product + mi_upconv_tail_fwd). */
/* mi_conv_d32_kind 1 / 3 (2-D 3 x 3) with the 2 x 2 max-pool of the result as a SECOND output (unet.py:198-249: conv -> BatchNorm ->
 * ReLU -> MaxPool2d(2, ceil_mode) - the un-pooled tensor is the skip connection): y (N, D, H, W, Co), y_pool (N, D, H / 2, W / 2, Co);
 * H, W multiples of 16; images as for mi_conv_d32_fwd_f32 / mi_conv_d64_fwd_f32.  A lane's accumulators of a row block are a 4 x 4
 * patch of one channel: the windows never leave the lane. */
int mi_conv_d32_fwd_pool_f32(const float* x, const void* wimg, const float* bias, float* y, float* y_pool, int relu, int N, int D, int H,
                             int W, int Ci, int Co, mi_stream_t stream);
/* ... with y a channel slice of a wider tensor (voxel v's Co channels at y + v * y_cstride): the skip connection written straight into
 * the concatenation buffer of the up-convolution block that consumes it (y = cat + Co_up, y_cstride = Co_up + Co), whose first Co_up
 * channels mi_conv_d32_upconv_fwd_f32 writes later - no concatenation pass at all.  y_pool stays dense. */
int mi_conv_d32_fwd_pool_strided_f32(const float* x, const void* wimg, const float* bias, float* y, int y_cstride, float* y_pool, int relu,
                                     int N, int D, int H, int W, int Ci, int Co, mi_stream_t stream);
/* dst[m][c0 : c0 + Cs] = src[m][:] over the M rows of a (M, Ct) tensor (channel counts and c0 multiples of 4): the encoder feature
 * into the concatenation buffer of an up-convolution block (torch.cat((up, enc), 1), unet.py:392) behind mi_conv_d32_upconv_fwd_f32. */
int mi_copy_channels_into(const float* src, int Cs, float* dst, int Ct, int c0, long M, mi_stream_t stream);
int mi_conv_d32_upconv_fwd_f32(const float* x, const void* wimg, const float* scale, const float* shift, float* out, int N, int H,
                               int W, int Ci, int Co, int Ho, int Wo, int cstride, mi_stream_t stream);
int mi_conv_d64_fwd_f32(const float* x, const void* wimg, const float* bias, float* y, int relu, int N, int D, int H, int W, int Ci,
                        int Co, mi_stream_t stream);
int mi_conv_d32_fwd_f32(const float* x, const void* wimg, const float* bias, float* y, int relu, int N, int D, int H, int W,
                        int Ci, int kind, mi_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Detector network glue (models/networks/unet.py, unet_small.py), channels-last.
 * ------------------------------------------------------------------------------------------ */
/* nn.MaxPool2d(k, ceil_mode=True) per image (unet.py:231-233): Ho = ceil(Hi/k); argmax (tap in the window,
 * may be NULL) feeds the backward. */
int mi_maxpool2d_ceil_fwd(const float* x, float* y, uint8_t* argmax, int N, int Hi, int Wi, int C, int k,
                          mi_stream_t stream);
int mi_maxpool2d_ceil_bwd(const float* dy, const uint8_t* argmax, float* dx, int N, int Hi, int Wi, int C,
                          int k, mi_stream_t stream);
/* nn.ConvTranspose2d(Ci, Co, 2, stride=2) (unet.py:155-160) = 1x1 conv to 4*Co columns [(a*2+b)*Co + co]
 * (mi_conv_fwd_f32) + this shuffle: y[n][2h+a][2w+b][co] = t[n][h][w][(a*2+b)*Co+co] + bias[co], cropped to
 * (Ho, Wo) <= (2H, 2W) (`autocrop`, unet.py:253-266).  bwd: the inverse scatter (zeros in the cropped rim). */
int mi_shuffle2x2_fwd(const float* t, const float* bias, float* y, int N, int H, int W, int Co, int Ho, int Wo,
                      mi_stream_t stream);
/* Inference tail of an up-convolution block in one pass (models/networks/unet.py:319-399: ConvTranspose2d(2, stride 2) -> BatchNorm2d
 * (eval) -> ReLU -> torch.cat with the encoder feature): out (N, Ho, Wo, Co + Ce) = cat(relu(scale[co] * shuffle(t) + shift[co]), enc);
 * t (N, H, W, 4*Co) is the 1 x 1 product of the transposed convolution, scale / shift the BatchNorm with the bias folded in. */
int mi_upconv_tail_fwd(const float* t, const float* scale, const float* shift, const float* enc, float* out, int N, int H,
                       int W, int Co, int Ce, int Ho, int Wo, mi_stream_t stream);
int mi_shuffle2x2_bwd(const float* dy, float* dt, int N, int H, int W, int Co, int Ho, int Wo,
                      mi_stream_t stream);
/* torch.cat((a, b), 1) (unet.py:385) over M rows, and its backward. */
int mi_concat_channels(const float* a, int Ca, const float* b, int Cb, float* out, long M, mi_stream_t stream);
int mi_split_channels(const float* dout, float* da, int Ca, float* db, int Cb, long M, mi_stream_t stream);
/* nn.Conv3d(C, K, (3,1,1), padding=(1,0,0), bias=False) with K <= 4 outputs: the `hm` head
 * (unet_small.py:55-62).  x (N,D,P,C), w [3][C][K], y (N,D,P,K), P = H*W. */
int mi_zhead_fwd(const float* x, const float* w, float* y, int N, int D, long P, int C, int K,
                 mi_stream_t stream);
/* its backward: dx (N,D,P,C) and dw [3][C][K], either may be NULL; 256 % C == 0 */
size_t mi_zhead_bwd_workspace_bytes(int N, int D, long P, int C, int K);
int mi_zhead_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, int N, int D, long P, int C,
                 int K, void* ws, size_t ws_bytes, mi_stream_t stream);

/* nn.BatchNorm3d / BatchNorm1d over rows [M][C] (moco_encoder_3d.py:170,184,199-205), split so a
 * SyncBN all-reduce of `sums` (2*C doubles: sum x, sum x^2) fits between stats and apply.
 * count = rows behind `sums` (global M under SyncBN).  save = mean[C], invstd[C].
 * gamma/beta NULL = affine=False.  running stats NULL = not tracked; num_batches_tracked (int64, may be
 * NULL) is incremented on the device by the same launch.  C % 4 == 0, 256 % (C/4) == 0.
 * y = act(bn(x) + res): res (may be NULL) is the residual branch of the 2-D BasicBlock
 * (simsiam_model_2d.py:485-502). */
size_t mi_colreduce_workspace_bytes(long M, int C);
int mi_bn_stats(const float* x, long M, int C, double* sums, void* ws, size_t ws_bytes,
                mi_stream_t stream);
int mi_bn_apply_fwd(const float* x, float* y, long M, int C, const double* sums, double count,
                    const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, long long* num_batches_tracked,
                    float* save_mean_invstd, const float* res, int relu, mi_stream_t stream);
/* The stem's BatchNorm3d + ReLU + MaxPool3d(3, 2, 1) (moco_encoder_3d.py:170-172) fused: relu(bn(x)) is never
 * written.  fwd: after mi_bn_stats (+ SyncBN all-reduce); sums == NULL = eval mode.  x (N,Di,Hi,Wi,C), pooled
 * (N,Do,Ho,Wo,C), argmax uint8.  bwd: mi_maxpool3d_bwd, then mi_bn_relu_bwd_{reduce,apply}_x. */
int mi_bn_relu_maxpool3d_fwd(const float* x, float* y, uint8_t* argmax, int N, int Di, int Hi, int Wi, int C, int k,
                             int stride, int pad, const double* sums, double count, const float* gamma,
                             const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                             long long* num_batches_tracked, float* save_mean_invstd, mi_stream_t stream);
/* Backward of relu(bn(x)) without the stored activation (mask recomputed from x); dy = mi_maxpool3d_bwd's output. */
int mi_bn_relu_bwd_reduce_x(const float* dy, const float* x, long M, int C, const float* save_mean_invstd,
                            const float* gamma, const float* beta, double* sums, void* ws, size_t ws_bytes,
                            mi_stream_t stream);
int mi_bn_relu_bwd_apply_x(const float* dy, const float* x, float* dx, long M, int C, const float* save_mean_invstd,
                           const float* gamma, const float* beta, const double* sums, double count, float* dgamma,
                           float* dbeta, mi_stream_t stream);
/* Small-M BatchNorm (M <= MI_BN_SMALL_MAX_ROWS: the BatchNorm1d layers of the projection MLPs,
 * moco_encoder_3d.py:199-205, and feature_3d's BatchNorm3d) in one launch each way; same results as the split
 * calls, which remain the path under SyncBN (the all-reduce sits between their halves). */
#define MI_BN_SMALL_MAX_ROWS 4096
int mi_bn_small_fwd(const float* x, float* y, long M, int C, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                    float* save_mean_invstd, const float* res, int relu, mi_stream_t stream);
int mi_bn_small_bwd(const float* dy, const float* x, const float* y, float* dx, long M, int C,
                    const float* save_mean_invstd, const float* gamma, int relu, float* dgamma, float* dbeta,
                    mi_stream_t stream);
/* global_avgpool(relu(bn(x))) in the launch of the small-M BatchNorm (nn.BatchNorm3d + ReLU + AdaptiveAvgPool3d(1) behind
 * feature_3d, models/networks/moco_encoder_3d.py:178-181,385-388): `pooled` (M / V, C) is the mean over the V consecutive
 * rows of each sample (V a power of two <= 64 dividing M); y = relu(bn(x)) is written as well - the backward reads its sign.
 * mi_bn_small_pool_bwd takes the gradient of `pooled`. */
int mi_bn_small_pool_fwd(const float* x, float* y, float* pooled, long M, int C, int V, const float* gamma,
                         const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                         long long* num_batches_tracked, float* save_mean_invstd, mi_stream_t stream);
int mi_bn_small_pool_bwd(const float* dpooled, const float* x, const float* y, float* dx, long M, int C, int V,
                         const float* save_mean_invstd, const float* gamma, float* dgamma, float* dbeta,
                         mi_stream_t stream);
int mi_bn_eval_fwd(const float* x, float* y, long M, int C, const float* running_mean,
                   const float* running_var, const float* gamma, const float* beta, float eps,
                   float* save_mean_invstd, const float* res, int relu, mi_stream_t stream);
/* backward: sums = {sum dy', sum dy'*xhat} with dy' = dy*(y>0) when relu; then
 * dx = gamma*invstd*(dy' - sums[0]/count - xhat*sums[1]/count), dgamma = sums[1], dbeta = sums[0]. */
int mi_bn_bwd_reduce(const float* dy, const float* x, const float* y, long M, int C,
                     const float* save_mean_invstd, int relu, double* sums, void* ws,
                     size_t ws_bytes, mi_stream_t stream);
int mi_bn_bwd_apply(const float* dy, const float* x, const float* y, float* dx, long M, int C,
                    const float* save_mean_invstd, const float* gamma, const double* sums,
                    double count, int relu, float* dgamma, float* dbeta, mi_stream_t stream);

/* mi_bn_bwd_apply for y = relu(bn(x) + residual) (cet_pick/models/networks/simsiam_model_2d.py:473-502, the end of a BasicBlock): the
 * gradient behind the ReLU, dres = dy * (y > 0), is what the residual branch receives - written by the same pass (no masking launch in
 * front of it); the statistics in `sums` are mi_bn_bwd_reduce's with relu = 1. */
int mi_bn_bwd_apply_res(const float* dy, const float* x, const float* y, float* dx, float* dres, long M, int C,
                        const float* save_mean_invstd, const float* gamma, const double* sums, double count,
                        float* dgamma, float* dbeta, mi_stream_t stream);
/* dgamma = sums[C..2C), dbeta = sums[0..C) from the LOCAL (pre all-reduce) backward sums: under
 * SyncBN the affine gradients stay per-rank and are averaged with the other gradients, exactly as
 * torch.nn.SyncBatchNorm does. */
int mi_bn_param_grads(const double* sums, int C, float* dgamma, float* dbeta, mi_stream_t stream);
/* column sum (bias gradient of nn.Linear, moco_encoder_3d.py:189): out[c] = sum_m dy[m][c] */
int mi_colsum(const float* dy, long M, int C, float* out, double* sums_scratch, void* ws,
              size_t ws_bytes, mi_stream_t stream);

/* nn.MaxPool3d(k, stride, pad) (moco_encoder_3d.py:172), argmax tap kept per element (uint8,
 * first maximum in (kd,kh,kw) scan order, as torch); backward routes dy to that element. */
int mi_maxpool3d_fwd(const float* x, float* y, uint8_t* argmax, int N, int Di, int Hi, int Wi,
                     int C, int k, int stride, int pad, mi_stream_t stream);
int mi_maxpool3d_bwd(const float* dy, const uint8_t* argmax, float* dx, int N, int Di, int Hi,
                     int Wi, int C, int k, int stride, int pad, mi_stream_t stream);
/* nn.AdaptiveAvgPool3d(1) (moco_encoder_3d.py:188): x [B][S][C] -> y [B][C] */
int mi_avgpool_fwd(const float* x, float* y, int B, int S, int C, mi_stream_t stream);
int mi_avgpool_bwd(const float* dy, float* dx, int B, int S, int C, mi_stream_t stream);
int mi_bias_add(float* y, const float* bias, long M, int C, mi_stream_t stream);
/* dst0 <- src0 and dst1 <- src1 (n floats each, n % 4 == 0, 16-byte aligned) in one launch: the two views of a batch
 * (trains/base_trainer.py:486-491: batch['input'], batch['input_aug']) into the step engine's static input buffers. */
int mi_copy_pair_f32(float* dst0, const float* src0, float* dst1, const float* src1, long n, mi_stream_t stream);
/* out = (dy + add) * (y > 0)   (ReLU backward; add may be NULL; n % 4 == 0) */
int mi_relu_mask(const float* dy, const float* y, const float* add, float* out, long n,
                 mi_stream_t stream);

/* F.normalize(x, dim=1) and the MoCo logits (models/moco.py:111-138):
 * logits[b] = [q_b.k_b, q_b.queue] / T, queue is [C][R]. */
int mi_l2norm_fwd(const float* x, float* y, float* inv_norm, int B, int C, mi_stream_t stream);
int mi_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int B, int C,
                  mi_stream_t stream);
int mi_moco_logits_fwd(const float* q, const float* k, const float* queue, float* logits, int B,
                       int C, int R, float T, mi_stream_t stream);
/* The same logits from the un-normalised projections (models/moco.py:113-138: q = normalize(encoder_q(im_q)), k =
 * normalize(encoder_k(im_k)), logits): q_hat (B, C), q_inv (B) = 1/|q| and k_hat (B, C) leave as by-products - the inputs
 * of mi_l2norm_bwd / mi_moco_logits_bwd and of the enqueue.  Rows bit-identical to mi_l2norm_fwd + mi_moco_logits_fwd. */
int mi_moco_logits_norm_fwd(const float* q_raw, const float* k_raw, const float* queue, float* logits, float* q_hat,
                            float* q_inv, float* k_hat, int B, int C, int R, float T, mi_stream_t stream);
int mi_moco_logits_bwd(const float* dlogits, const float* k, const float* queue, float* dq, int B,
                       int C, int R, float T, mi_stream_t stream);
/* SimSiam loss pieces (trains/tomo_simsiam_trainer.py:28-40) on L2-normalised rows:
 * out = mean_b(a_b . b_b) (nn.CosineSimilarity(dim=1)(p, z).mean() once p, z are normalised), its
 * gradient da = grad_out/B * b, and output_std = torch.std(x, 0).mean(). */
int mi_rowdot_mean_fwd(const float* a, const float* b, float* out, int B, int C, mi_stream_t stream);
int mi_rowdot_mean_bwd(const float* b, const float* grad_out, float* da, int B, int C, mi_stream_t stream);
int mi_column_std_mean(const float* x, float* out, int B, int C, mi_stream_t stream);
/* nn.CrossEntropyLoss against label 0 (trains/tomo_moco_trainer.py:52,73; models/moco.py:141): loss = mean_b(logsumexp(l_b) - l_b[0])
 * in ONE launch (a workgroup per row; the last one to finish takes the mean, in row order), row_loss[B] and
 * row_lse[2B] (the rows' maxima, then the logs of their sums) scratch / kept for the backward pass; the backward reads the upstream gradient from the device (no host
 * value, no extra scaling launch): dlogits = grad_loss * (softmax - onehot0) / B.
 * counter: the arrival counter of the "last workgroup" - ONE 4-byte word owned by the caller, zero before the first call and
 * left zero by every call; give each stream (and each model) its own.  NULL: a process-wide word - one call at a time per device. */
int mi_ce_label0_fwd(const float* logits, float* loss, float* loss_copy /* may be NULL: a second place for the value */,
                     float* row_loss, float* row_lse, int B, int n, unsigned* counter, mi_stream_t stream);
int mi_ce_label0_bwd(const float* logits, const float* row_lse, const float* grad_loss, float* dlogits, int B, int n,
                     mi_stream_t stream);

/* Data gradient of the encoder's stride-2 3x3x3 convolutions (moco_encoder_3d.py:55-84,257-272: layer2.0.conv1 64 -> 128 on 8^3,
 * layer3.0.conv1 128 -> 256 on 4^3 - and on 8^3, the 64^3 crops' layer3.0; padding 1) with the block's 1x1 stride-2 shortcut folded in - one launch per block instead of
 * two data-gradient launches and their split-K reduces (csrc/conv_s2.hip):
 *   dx (N, Gi, Gi, Gi, Ci) = (conv_dgrad(dh; w) [+ conv1x1_dgrad(dout; w_ds)] + res) * (mask > 0)
 * dh / dout: (N, Gi/2, Gi/2, Gi/2, Co); w: [27][Ci][Co], w_ds: [Ci][Co] (kernel layouts); dout and w_ds are given together or
 * both NULL; res / mask (shape of dx) may be NULL.  `ws`: mi_conv3d_s2_dgrad_workspace_bytes(Ci, Co) bytes - the call cuts the
 * weight images into it.  mi_conv3d_s2_dgrad_usable: 1 for the three shapes above (bf16x3 arithmetic), else 0 (the caller keeps
 * mi_conv_dgrad_f32). */
int mi_conv3d_s2_dgrad_usable(int N, int Gi, int Ci, int Co);
size_t mi_conv3d_s2_dgrad_workspace_bytes(int Ci, int Co);
int mi_conv3d_s2_dgrad_f32(const float* dh, const float* dout, const float* w, const float* w_ds, float* dx, const float* res,
                           const float* mask, int N, int Gi, int Ci, int Co, void* ws, size_t ws_bytes, mi_stream_t stream);

/* Forward of the same block front in one launch (csrc/conv_s2.hip): hmid (N, Gi/2.., Co) = relu(conv3d(x; w [27][Ci][Co], k 3,
 * stride 2, pad 1)) and the 1x1 stride-2 shortcut r (N, Gi/2.., Co) = conv3d(x; w_ds [Ci][Co]) - replaces two mi_conv_fwd_f32
 * calls (models/networks/moco_encoder_3d.py:66-69,78-79: conv1 + relu, downsample).  `ws`: mi_conv3d_s2_fwd_workspace_bytes(Ci, Co)
 * bytes - the call cuts the weight image into it.  mi_conv3d_s2_fwd_usable: 1 for the two encoder shapes, else 0. */
int mi_conv3d_s2_fwd_usable(int N, int Gi, int Ci, int Co);
size_t mi_conv3d_s2_fwd_workspace_bytes(int Ci, int Co);
int mi_conv3d_s2_fwd_f32(const float* x, const float* w, const float* w_ds, float* hmid, float* r, int N, int Gi, int Ci, int Co,
                         void* ws, size_t ws_bytes, mi_stream_t stream);

/* Caller-kept images of the stride-2 fronts: mi_conv3d_s2_prep cuts the images of n fronts in one launch per 8 (host arrays of
 * device pointers; w[i] [27][Ci][Co], w_ds[i] [Ci][Co] - may be NULL only for a data-gradient image of a block without
 * shortcut -, img[i] of mi_conv3d_s2_fwd_workspace_bytes / mi_conv3d_s2_dgrad_workspace_bytes bytes, dgrad[i] 0 / 1); the _img_
 * calls are mi_conv3d_s2_fwd_f32 / mi_conv3d_s2_dgrad_f32 without the image build (a training loop cuts the images once per
 * weight update, behind its SGD / momentum kernel, instead of in front of every call). */
int mi_conv3d_s2_prep(const float* const* w, const float* const* w_ds, void* const* img, const int* ci, const int* co,
                      const int* dgrad, int n, mi_stream_t stream);
int mi_conv3d_s2_fwd_img_f32(const float* x, const void* img, float* hmid, float* r, int N, int Gi, int Ci, int Co,
                             mi_stream_t stream);
int mi_conv3d_s2_dgrad_img_f32(const float* dh, const float* dout, const void* img, float* dx, const float* res,
                               const float* mask, int N, int Gi, int Ci, int Co, mi_stream_t stream);

/* models/moco.py:31-39: k <- m*k + (1-m)*q over a flat parameter arena (16-B aligned). */
int mi_ema_update(float* k, const float* q, float m, long n, mi_stream_t stream);
/* torch.optim.SGD (moco_main.py:79, no momentum): p <- p - lr*(grad_scale*g + wd*p).  lr_dev (device float,
 * may be NULL -> lr) lets a captured graph follow the schedule; grad_scale = 1 / world size when g holds the sum of the
 * data-parallel ranks' gradients (DistributedDataParallel's averaging, moco_main.py:44-66), 1 otherwise. */
int mi_sgd_step(float* p, const float* g, const float* lr_dev, float lr, float weight_decay, float grad_scale, long n,
                mi_stream_t stream);
/* Round 6: p <- p - lr (grad_scale (g + g2) + wd p): the step of a model whose two views wrote their parameter gradients into two
 * arenas (trains/simsiam_engine.py; simsiam_main.py:65 SGD over both views' accumulated gradients). */
int mi_sgd_step2(float* p, const float* g, const float* g2, const float* lr_dev, float lr, float weight_decay, float grad_scale, long n,
                 mi_stream_t stream);
/* sums[i] += *src_i for the non-NULL device scalars a, b, c, d (the per-step loss meters of trains/base_trainer.py:514-530, kept on
 * the device and read once per print interval). */
int mi_scalar_accumulate(float* sums, const float* a, const float* b, const float* c, const float* d, mi_stream_t stream);
/* models/moco.py:41-52: queue[:, ptr:ptr+B] = keys.T; ptr = (ptr+B) % R, ptr read and advanced on
 * the device (no host sync).  R % B == 0 as the reference asserts. */
int mi_queue_enqueue(float* queue, int64_t* queue_ptr, const float* keys, int B, int C, int R,
                     mi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Detector-training losses, cet_pick/models/loss.py.  `pred` is the clamped sigmoid
 * heat-map, `gt` the label map (1 positive, (-1,1) soft, -1 unlabeled).  Each forward writes the scalar loss
 * (device float) and `sums` (11 doubles: the 8 partial sums, loss, PU branch flag, n) that the backward
 * reads; nothing synchronises.  ws: mi_voxel_loss_workspace_bytes(n).
 * ------------------------------------------------------------------------------------------ */
size_t mi_voxel_loss_workspace_bytes(long n);
/* `_pu_neg_loss(pred, gt, tau, beta, gamma)` loss.py:255-308 (the `< -beta` branch is taken on the device). */
int mi_pu_focal_loss_fwd(const float* pred, const float* gt, long n, double tau, double beta, double* sums,
                         float* loss, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_pu_focal_loss_bwd(const float* pred, const float* gt, long n, double tau, const double* sums,
                         const float* dloss, float* dpred, mi_stream_t stream);
/* `_neg_loss(pred, gt)` loss.py:378-411 (FocalLoss). */
int mi_focal_loss_fwd(const float* pred, const float* gt, long n, double* sums, float* loss, void* ws,
                      size_t ws_bytes, mi_stream_t stream);
int mi_focal_loss_bwd(const float* pred, const float* gt, long n, const double* sums, const float* dloss,
                      float* dpred, mi_stream_t stream);
/* `_pu_ge_loss(pred, gt, tau, FocalLoss(), slack, entropy_penalty)` loss.py:215-253 (PUGELoss :327-337, the trainer's --ge):
 *   loss = focal(labelled voxels) + slack * pen.  With U = {gt == -1}, N = |U|, mu = sum_U p, v = sum_U p (1 - p), w = v + 1e-7,
 *   s_k = -(mu - k)^2 / (2 w), q = softmax(s) over k = 0 .. N, b_k = log Binom(k; N, tau) (lgamma form), B = sum_k q_k b_k:
 *   pen = -B + [entropy_penalty > 0] entropy_penalty / 2 (log v + log 2 pi + 1)            (v = 0 then gives -inf, as the reference)
 *   g_mu = -sum_k q_k (b_k - B)(k - mu) / w,  g_v = -sum_k q_k (b_k - B)(k - mu)^2 / (2 w^2) + [..] entropy_penalty / (2 v)
 *   d loss / d p_i = slack (g_mu + g_v (1 - 2 p_i)) on U; the focal gradient (mi_focal_loss_bwd's) on the labelled voxels.
 * The count sum runs in double on the device over the window of counts whose term does not underflow against the largest one
 * (a float64 softmax over all N + 1 counts adds exact zeros outside it); N, mu and v are never read on the host, nothing
 * synchronises.  N = 0: pen = 0.  tau outside (0, 1): MI_E_ARG, nothing launched.
 * `sums`, 16 doubles, written by the forward and read by the backward:
 *   [0] #positive  [1] #soft  [2] N = #unlabeled  [3] sum log(p)(1-p)^2 [positive]  [4] sum log(1-p) p^2 (1-g)^4 [soft]
 *   [5] mu  [6] v  [7] focal  [8] loss  [9] pen  [10] n  [11] B  [12] g_mu  [13] g_v  [14], [15] first and last count walked
 * ws: mi_pu_ge_loss_workspace_bytes(n). */
size_t mi_pu_ge_loss_workspace_bytes(long n);
int mi_pu_ge_loss_fwd(const float* pred, const float* gt, long n, double tau, double slack, double entropy_penalty,
                      double* sums, float* loss, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_pu_ge_loss_bwd(const float* pred, const float* gt, long n, double slack, const double* sums, const float* dloss,
                      float* dpred, mi_stream_t stream);
/* `ConsistencyLoss` loss.py:701-712: mean((a-b)^2); db may be NULL. */
int mi_mse_loss_fwd(const float* a, const float* b, long n, double* sums, float* loss, void* ws,
                    size_t ws_bytes, mi_stream_t stream);
int mi_mse_loss_bwd(const float* a, const float* b, long n, const double* sums, const float* dloss, float* da,
                    float* db, mi_stream_t stream);
/* `UnbiasedConLoss.forward` loss.py:594-699 without the (2N)^2 matrix.  feat [n2][dim] (both views stacked,
 * n2 = 2N, row i and row i +- N are the two views of a voxel; dim 32 or 64), cls[n2]: bit 0 positive label,
 * bit 1 "other" (label < thresh).  With S = feat feat^T * inv_T, m_i = max_j S_ij and
 * E_ij = exp((S_ij - m_i) * [i != j]) (loss.py:615-624) the forward returns per row
 *   rowmax = m_i, s_all = sum_j E_ij, s_pos = sum_j E_ij [pos j], s_other = sum_j E_ij [other j], e_pair = E_i,pair(i)
 * and the backward, given the gradients of those four sums, d(loss)/d(feat) (m_i is detached like
 * `logits_max_all.detach()`). */
int mi_ucl_rowsums_fwd(const float* feat, const uint8_t* cls, int n2, int dim, float inv_T, float* rowmax,
                       float* s_all, float* s_pos, float* s_other, float* e_pair, mi_stream_t stream);
/* The gradient forms both terms of a similarity tile at once (S is symmetric: one product, one contraction; MI_UCL_BWD_SPLIT=1: the two
 * launches of rounds 2-5) and, where the row maxima lie within 2^16 of each other - always for L2-normalised features - takes ONE
 * exponential per similarity; decided on the device from `range` (2 floats of scratch; NULL, dim 64 or MI_UCL_BWD_TWO_EXP=1: the
 * two-exponential form). */
int mi_ucl_rowsums_bwd_ranged(const float* feat, const uint8_t* cls, int n2, int dim, float inv_T, const float* rowmax,
                              const float* g_all, const float* g_pos, const float* g_other, const float* g_pair, float* dfeat,
                              float* range, mi_stream_t stream);
/* `SupConLossV2_more.forward` loss.py:759-818 (the trainer's --pn) around the row sums above: the O(N) part, doubles throughout.
 * cls bit 0: pos (label > thresh), bit 1: un (label < thresh); P2 = #pos, U = #un over the n2 rows, G = sum_{j pos} feat_j,
 * m_i = rowmax, Z_i = s_all of mi_ucl_rowsums_fwd on the same feat / cls / inv_T:
 *   loss = -1/P2 sum_{i pos} [(f_i.G - f_i.f_i) inv_T - (P2 - 1) m_i] / P2 - log Z_i   -  1/U sum_{i un} f_i.f_pair(i) inv_T - m_i - log Z_i
 * The forward writes loss (device float), g_all[i] = d loss / d Z_i (1 / (P2 Z_i) on pos rows, 1 / (U Z_i) on un rows, 0 elsewhere)
 * and `sums`, 72 doubles: [0] P2  [1] U  [2] sum over pos rows  [3] sum over un rows  [4] loss  [8 + c] G[c].  P2 = 0 or U = 0: the
 * loss is not finite (the caller checks its labels).  The backward takes dfeat = mi_ucl_rowsums_bwd_ranged(g_all, 0, 0, 0) and leaves
 *   dfeat = *dloss (dfeat - [pos k] 2 (G - f_k) inv_T / P2^2 - [un k] 2 f_pair(k) inv_T / U).
 * Nothing synchronises.  ws: mi_supcon_pn_rows_workspace_bytes(n2). */
size_t mi_supcon_pn_rows_workspace_bytes(int n2);
int mi_supcon_pn_rows_fwd(const float* feat, const uint8_t* cls, int n2, int dim, float inv_T, const float* rowmax,
                          const float* s_all, float* g_all, double* sums, float* loss, void* ws, size_t ws_bytes,
                          mi_stream_t stream);
int mi_supcon_pn_rows_bwd(const float* feat, const uint8_t* cls, int n2, int dim, float inv_T, const double* sums,
                          const float* dloss, float* dfeat, mi_stream_t stream);

/* k-means over embeddings (reference plot_2d.py: faiss.Kmeans(d, 256, niter=300)), DESIGN.md 4.9.  x (n, d) fp32 rows,
 * centroids (k, d) fp32, 1 <= d <= 512, 2 <= k <= 1024, k <= n < 2^31 (MI_E_UNSUPPORTED outside; the size entries return 0).
 * Rows are addressed with 64-bit offsets: n x d may exceed 2 GiB.  One arithmetic: bf16x3 on the matrix cores
 * (MI_CONV_ARITH is not consulted).
 *   mi_kmeans_prep    image (mi_kmeans_image_bytes, 16-byte aligned) = the centroids' bf16x3 cut in MFMA operand order + |c_j|^2
 *   mi_kmeans_xnorm   xnorm[i] = |x_i|^2
 *   mi_kmeans_assign  labels[i] = argmin_j |x_i|^2 + (|c_j|^2 - 2 x_i.c_j), the LOWEST j on ties; dist[i] = that minimum,
 *                     clamped at 0.  Leaves per-workgroup sums of dist in ws for the mi_kmeans_update that follows.
 *   mi_kmeans_update  counts[j] and centroids[j] = mean of the rows with labels[i] == j (labels outside [0, k) are left out),
 *                     deterministic: stable counting sort of the indices, sums of 64 sorted positions in position order, those
 *                     in segment order in fp64.  Then, on the device, empty clusters in ascending index: the donor is the
 *                     cluster with the most points at that moment (lowest index on ties); the empty cluster takes the donor's
 *                     centroid with component m times 1 + 1/1024 (m even) or 1 - 1/1024 (m odd), the donor the opposite; of the
 *                     donor's count n the empty cluster takes n / 2, the donor keeps n - n / 2 (counts[] holds the split
 *                     values).  obj (may be NULL): obj[0] = sum of dist of the mi_kmeans_assign that last wrote ws (same n, d,
 *                     k).  nsplit (may be NULL): nsplit[0] += number of empty clusters served.
 * ws: mi_kmeans_workspace_bytes(n, d, k), 16-byte aligned, shared by assign and update. */
size_t mi_kmeans_image_bytes(int d, int k);
size_t mi_kmeans_workspace_bytes(long n, int d, int k);
int mi_kmeans_prep(const float* centroids, int d, int k, void* image, mi_stream_t stream);
int mi_kmeans_xnorm(const float* x, long n, int d, float* xnorm, mi_stream_t stream);
int mi_kmeans_assign(const float* x, const float* xnorm, const void* image, long n, int d, int k, int32_t* labels,
                     float* dist, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_kmeans_update(const float* x, const int32_t* labels, long n, int d, int k, float* centroids, int32_t* counts,
                     float* obj, int32_t* nsplit, void* ws, size_t ws_bytes, mi_stream_t stream);

/* Exact k-nearest-neighbour search (reference utils/memory_bank.py: faiss.IndexFlatIP, matmul + topk), DESIGN.md 4.11.
 * q (m, d) and x (n, d) fp32 rows, 1 <= d <= 512, 1 <= k <= 128, 1 <= m < 2^31, k <= n < 2^31 (k + 1 <= n with exclude_self),
 * 0 <= n_split <= 32 (MI_E_UNSUPPORTED outside; the size entries return 0).  Rows are addressed with 64-bit offsets: n x d may
 * exceed 2 GiB.  One arithmetic: bf16x3 on the matrix cores (MI_CONV_ARITH is not consulted).
 *   mi_knn_search  out_index (m, k) int32 = the k best rows of x for every row of q, best first, out_value (m, k) fp32 their
 *                  values.  MI_KNN_IP: the value is q.x, larger is better.  MI_KNN_L2: the value is |q|^2 + (|x|^2 - 2 q.x)
 *                  evaluated in that order and clamped at 0, smaller is better.  Equal values: the LOWEST index first.
 *                  exclude_self: column j is left out for query row j (a set searched against itself).  The database is cut
 *                  once per call into its MFMA operand image (mi_knn_image_bytes(n, d) of ws); the m x n values are never
 *                  stored: a workgroup keeps the running top k of its query rows and takes only the values that beat a row's
 *                  k-th.  The columns are divided into n_split parts (0: the library chooses) whose partial results a second
 *                  launch merges; the result does not depend on n_split, and the same inputs give the same bytes.  A NaN value
 *                  counts as the worst.
 * ws: mi_knn_workspace_bytes(m, n, d, k, exclude_self, n_split) (the image included), 16-byte aligned; q and x 16-byte aligned
 * when d is a multiple of 4. */
#define MI_KNN_IP 0
#define MI_KNN_L2 1
size_t mi_knn_image_bytes(long n, int d);
size_t mi_knn_workspace_bytes(long m, long n, int d, int k, int exclude_self, int n_split);
int mi_knn_search(const float* q, const float* x, long m, long n, int d, int k, int metric, int exclude_self, int n_split,
                  int32_t* out_index, float* out_value, void* ws, size_t ws_bytes, mi_stream_t stream);

/* Exact t-SNE over a k-nearest-neighbour graph (reference plot_2d.py --mode tsne: sklearn.manifold.TSNE, 2 components, one
 * degree of freedom), DESIGN.md 4.12.  2 <= n <= 2^24, 1 <= k <= 127, k <= n - 1, 0 <= n_split <= 32 (MI_E_UNSUPPORTED
 * outside, nothing launched; the size entry returns 0).  Edge e = i k + c of the graph runs from row i to row index[e].
 *   mi_tsne_affinities  dist (n, k) fp32, ascending in a row: per row sklearn's _binary_search_perplexity in double (bisection
 *                       on beta, doubling while unbounded, at most 100 steps, until |H(beta) - ln perplexity| <= 1e-5), the
 *                       row's smallest distance subtracted first.  out_beta (n) = beta as fp32, out_p (n, k) = exp(-beta d) /
 *                       sum at that fp32 value.  A row of equal distances gives 1 / k.  1 <= perplexity <= k.
 *   mi_tsne_gradient    y (n, 2) fp32; index, p (n, k): the graph and its conditional affinities; rev_ptr (n + 1), rev_edge
 *                       (n k): the ids of the edges that END in row i are rev_edge[rev_ptr[i] .. rev_ptr[i + 1]), ascending.
 *                       The joint affinity of a pair is P = (p[i -> j] + p[j -> i]) / 2n, a missing direction counting 0; the
 *                       rows of index hold distinct neighbours.  With q_ij = 1 / (1 + |y_i - y_j|^2) and Z = sum over i != j
 *                       of q_ij (out_z): out_grad_i = 4 (exaggeration sum_j P_ij q_ij (y_i - y_j) - sum_{j != i} q_ij^2
 *                       (y_i - y_j) / Z), and out_kl (may be NULL: not computed) = sum over the pairs with P > 0 of
 *                       P ln(P Z / q), without the exaggeration.  The all-pairs sums are taken in fp32 over tiles of 128
 *                       points and in double above that; the j range is divided into n_split parts (0: chosen from n alone)
 *                       merged in split order.  No floating-point atomics: the same inputs and the same n_split give the same
 *                       bytes.  Edges that point outside [0, n) and edge ids outside [0, n k) are passed over.
 *   mi_tsne_update      sklearn's _gradient_descent step on the 2n components: gains + 0.2 where velocity grad < 0, gains 0.8
 *                       elsewhere, floored at min_gain; velocity = momentum velocity - lr (grad gains); y += velocity.  Every
 *                       product and sum is rounded once.
 * ws: mi_tsne_workspace_bytes(n, k, n_split), 16-byte aligned. */
int mi_tsne_affinities(const float* dist, long n, int k, float perplexity, float* out_p, float* out_beta, mi_stream_t stream);
size_t mi_tsne_workspace_bytes(long n, int k, int n_split);
int mi_tsne_gradient(const float* y, const int32_t* index, const float* p, const int32_t* rev_ptr, const int32_t* rev_edge, long n,
                     int k, float exaggeration, int n_split, float* out_grad, float* out_z, float* out_kl, void* ws,
                     size_t ws_bytes, mi_stream_t stream);
int mi_tsne_update(float* y, const float* grad, float* velocity, float* gains, long n, float momentum, float lr, float min_gain,
                   mi_stream_t stream);

/* UMAP over a k-nearest-neighbour graph (reference plot_2d.py --mode umap: umap.UMAP, 2 components), in its epoch-synchronous
 * form, DESIGN.md 4.14.  k is the number of COLUMNS of the graph, n_neighbors - 1 (UMAP counts the point itself).  1 <= k <= 127,
 * n >= k + 2, n k < 2^31 (MI_E_UNSUPPORTED outside, nothing launched; mi_umap_check is that test alone, on the host).  Edge
 * e = i k + c runs from row i to row index[e]; rev_ptr, rev_edge as mi_tsne_gradient takes them.
 *   mi_umap_smooth_knn  dist2 (n, k) fp32 squared distances: d = sqrt as fp32; per row, in double, rho = the smallest positive d
 *                       (0 where there is none) and sigma by bisection from 1 (doubling while unbounded, at most 64 steps) until
 *                       |sum_c (d_c > rho ? exp(-(d_c - rho) / sigma) : 1) - log2(k + 1)| < 1e-5, then floored at 1e-3 times the
 *                       row's mean distance sum_c d_c / (k + 1), or at 1e-3 mean_all where rho = 0.  out_rho, out_sigma (n)
 *                       fp32; out_w (n, k) = exp(-max(0, d - rho) / sigma) at the double sigma.
 *   mi_umap_union       per directed edge: out_wsym = a + b - a b with a = w[e] and b the weight of the opposite edge, 0 where
 *                       there is none; out_mutual (n k bytes) = 1 where it exists.  With wmax (one DEVICE float, the largest
 *                       wsym; NULL: out_eps is not written) out_eps (n k doubles) = wmax / wsym, +inf for an edge with
 *                       wsym < wmax / n_epochs.  An edge that points outside [0, n) or at its own row gets 0, 0, +inf.
 *   mi_umap_epoch       epoch `epoch` of n_epochs, 1-based, alpha = 1 - (epoch - 1) / n_epochs.  The incident pairs of vertex i
 *                       are its forward edges (slot = column) and then the edges that end in it and have mutual = 0, in
 *                       ascending edge id (slots k, k + 1, ...).  A pair with spacing eps fires iff floor(epoch / eps) >
 *                       floor((epoch - 1) / eps); a firing adds 2 clip(c (y_i - y_j)), c = -2 a b d2^(b - 1) / (a d2^b + 1) (0 at
 *                       d2 = 0), and for t = 0..4 the negative v = mulhi(word, n), word = philox4x32_10(i, slot, epoch, t / 4;
 *                       seed)[t % 4]: nothing for v = i, +4 on both components at d2 = 0, else clip(2 b / ((0.001 + d2) (a d2^b
 *                       + 1)) (y_i - y_v)); clip to [-4, 4] per component.  y_out_i = fp32(y_in_i + alpha sum), every term
 *                       and the sum in double from y_in alone; y_out may not alias y_in.  No floating-point atomics: the same
 *                       inputs give the same bytes.  Edge ids and destinations outside their range are passed over.
 * The label-supervised map (umap.UMAP.fit_transform(x, y) with a categorical target), DESIGN.md 4.16.  label (n) int32, any
 * negative value: unknown.  s(e) = wsym[e] f, f = f_unknown where an end of the edge is unknown, f_far where the labels of its
 * ends differ, 1 where they are equal; both factors are computed by the caller (exp(-1), exp(-2.5 / (1 - target_weight))).
 *   mi_umap_rowmax      out_rowmax (n doubles): m_i = the largest s over the k forward edges of row i and the edges
 *                       rev_edge[rev_ptr[i] .. rev_ptr[i + 1]) that end in it; 0 where there is none.  An edge that points
 *                       outside [0, n) or at its own row contributes 0.
 *   mi_umap_supervise   per directed edge i -> j: out_wsup = p + q - p q in double, stored as fp32, p = s / (m_i or 1),
 *                       q = s / (m_j or 1) with rowmax as mi_umap_rowmax wrote it; wmax, n_epochs, out_eps as in mi_umap_union,
 *                       on out_wsup.  An edge that points outside [0, n) or at its own row gets 0, +inf.  n_epochs < 1:
 *                       MI_E_UNSUPPORTED. */
int mi_umap_check(long n, int k);
int mi_umap_smooth_knn(const float* dist2, long n, int k, double mean_all, float* out_rho, float* out_sigma, float* out_w,
                       mi_stream_t stream);
int mi_umap_union(const int32_t* index, const float* w, const int32_t* rev_ptr, const int32_t* rev_edge, long n, int k,
                  const float* wmax, int n_epochs, float* out_wsym, uint8_t* out_mutual, double* out_eps, mi_stream_t stream);
int mi_umap_rowmax(const int32_t* index, const float* wsym, const int32_t* label, const int32_t* rev_ptr, const int32_t* rev_edge,
                   long n, int k, double f_far, double f_unknown, double* out_rowmax, mi_stream_t stream);
int mi_umap_supervise(const int32_t* index, const float* wsym, const int32_t* label, const double* rowmax, long n, int k,
                      double f_far, double f_unknown, const float* wmax, int n_epochs, float* out_wsup, double* out_eps,
                      mi_stream_t stream);
int mi_umap_epoch(const float* y_in, float* y_out, const int32_t* index, const int32_t* rev_ptr, const int32_t* rev_edge,
                  const uint8_t* mutual, const double* eps, long n, int k, int epoch, int n_epochs, double a, double b, uint64_t seed,
                  mi_stream_t stream);

/* The spectral start of the UMAP map (umap.UMAP's init="spectral"), DESIGN.md 4.15: the kernels of an eigen-solver over the graph
 * mi_umap_epoch walks.  n, k, index, rev_ptr, rev_edge, mutual, eps as there (mi_umap_check's range; MI_E_UNSUPPORTED outside, nothing
 * launched); wsym as mi_umap_union writes it.  The incident list of vertex i: its forward edges with finite eps, then the edges that
 * end in it with mutual = 0 and finite eps; the weight of an entry is wsym of that directed edge.  Edge ids and destinations
 * outside their range, and edges from a vertex to itself, are passed over.  All sums in double in a fixed order, no
 * floating-point atomics: the same inputs give the same bytes.
 *   mi_graph_components  one sweep of min-label propagation with pointer jumping: label_out_i = the smallest label_in among i and
 *                        its incident vertices, followed through label_in down to a vertex that is its own label; *changed (one
 *                        device int, zeroed by the caller) is set to 1 when a label moved.  Start from label_i = i and repeat, the
 *                        two buffers swapped, until *changed stays 0: every vertex then holds the smallest id of its component.
 *                        label_out may not alias label_in.
 *   mi_spectral_degree   out_deg_i = the sum of the incident weights, out_dis_i = 1 / sqrt(deg_i) (0 where deg_i = 0), n doubles.
 *   mi_spectral_spmv     y = A x over the rows [row0, row0 + nrows), A = D^-1/2 W D^-1/2 restricted to that range (entries that
 *                        leave it are passed over): x and y hold nrows doubles, element 0 is row row0; y may not alias x.
 *   mi_spectral_dots     c_v = sum_i Q[v ldq + i] w_i for v < m: 1 <= m <= 4096 vectors of 1 <= n < 2^31 doubles, ldq >= n.  Partial
 *                        sums of 2048 elements, added in order; ws: mi_spectral_workspace_bytes(m, n) (0 = unsupported sizes).
 *   mi_spectral_orth     c = Q^T w as mi_spectral_dots, then w = w - Q c with the vectors taken in order.  w outside Q.
 *   mi_spectral_combine  w = beta w - Q c (beta = 0: w is not read).  w outside Q. */
int mi_graph_components(const int32_t* index, const double* eps, const uint8_t* mutual, const int32_t* rev_ptr, const int32_t* rev_edge,
                        long n, int k, const int32_t* label_in, int32_t* label_out, int32_t* changed, mi_stream_t stream);
int mi_spectral_degree(const int32_t* index, const float* wsym, const double* eps, const uint8_t* mutual, const int32_t* rev_ptr,
                       const int32_t* rev_edge, long n, int k, double* out_deg, double* out_dis, mi_stream_t stream);
int mi_spectral_spmv(const int32_t* index, const float* wsym, const double* eps, const uint8_t* mutual, const int32_t* rev_ptr,
                     const int32_t* rev_edge, long n, int k, const double* dis, const double* x, double* y, long row0, long nrows,
                     mi_stream_t stream);
size_t mi_spectral_workspace_bytes(int m, long n);
int mi_spectral_dots(const double* Q, long ldq, int m, long n, const double* w, double* c, void* ws, size_t ws_bytes,
                     mi_stream_t stream);
int mi_spectral_orth(const double* Q, long ldq, int m, long n, double* w, double* c, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_spectral_combine(const double* Q, long ldq, int m, long n, const double* c, double* w, double beta, mi_stream_t stream);

/* 3-D visualisation of the exploration map (reference visualize_3dhm.py, and the colour step of plot_2d.py), DESIGN.md 4.13.
 * Volumes are (Z, R, C) row-major and addressed with 64-bit offsets; Z R C / 256 < 2^31 (MI_E_UNSUPPORTED above).
 *   mi_vis_sample_colours  y01 (n, 2) fp32, table (W, H, 3) uint8: out (n, 3) = table[ix, iy] with ix = clamp(rint(x (W - 1)), 0,
 *                          W - 1) on the double product (Python's round: half to even), iy likewise with H; a NaN samples 0.
 *   mi_vis_slice_bytes     x [n_slices][slice_elems] fp32, stats as mi_vol_stats writes them: out = the byte
 *                          rint(clip(255 ((x - mean) / std - mi) / (ma - mi), 0, 255)) of every voxel, in double; a slice whose
 *                          deviation is not > 0 gives 0 (the reference casts NaN there).
 *   mi_vis_gauss_u8        out (Z, R, C, 3) uint8 = scipy.ndimage.gaussian_filter of the three equal channels of in (Z, R, C)
 *                          uint8, bit for bit: four passes (z, rows, columns, channels) with the 7 weights `weights7` (a HOST
 *                          array of doubles, symmetric: scipy's _gaussian_kernel1d(sigma, 0, 3)), `reflect` borders, each
 *                          pass summed in double in scipy's order without FMA and truncated to a byte.  in may not alias out.
 *   mi_vis_paint           picks_xyz (n, 3) int32 (column, row, slice) in input order, colours (n, 3) uint8, slot_of_slice (Z)
 *                          int32: the plane of `index` (n_slots, R, C) that belongs to a slice, -1 for a slice that is to stay
 *                          zero.  Writes the slices [z0, z0 + nz) of out (Z, R, C, 3): a pixel of slice s takes the colour of the
 *                          LAST pick i with |z_i - s| <= 2 whose disc dx^2 + dy^2 <= (12 - |z_i - s|)^2 around (column, row)
 *                          holds it, 0 where there is none.  index is scratch, zeroed here (atomic max of i + 1: the result does
 *                          not depend on the arrival order); slots of slices outside the slab are not touched by the picks.
 * ws of mi_vis_gauss_u8: mi_vis_gauss_workspace_bytes(Z, R, C).  The word-wide forms run when C is a multiple of 4 and the
 * buffers are 4-byte aligned, the byte-wide forms otherwise; both give the same bytes. */
int mi_vis_sample_colours(const float* y01, long n, const uint8_t* table, int W, int H, uint8_t* out, mi_stream_t stream);
int mi_vis_slice_bytes(const float* x, long n_slices, long slice_elems, const double* stats, double mi, double ma, uint8_t* out,
                       mi_stream_t stream);
size_t mi_vis_gauss_workspace_bytes(long Z, long R, long C);
int mi_vis_gauss_u8(const uint8_t* in, int Z, int R, int C, const double* weights7, uint8_t* out, void* ws, size_t ws_bytes,
                    mi_stream_t stream);
int mi_vis_paint(const int32_t* picks_xyz, const uint8_t* colours, long n, const int32_t* slot_of_slice, int n_slots, int Z,
                 int R, int C, int z0, int nz, int32_t* index, uint8_t* out, mi_stream_t stream);

/* The pictures of the 2-D map and the thumbnails of the picks (reference plot_2d.py:96-103, :121-218), DESIGN.md 4.18.
 *   mi_plot_select       y01 (n, 2) fp32, finite.  The reference's filter in input order: `shown` starts as [y01[0]]; pick i
 *                        is skipped when min over shown of fl(fl(dx dx) + fl(dy dy)) < thr (float32, dx = fl(x_i - x_j)),
 *                        and is appended to shown and to shown_idx otherwise.  thr is a SQUARED distance; a distance equal
 *                        to thr does not block; with thr > 0 pick 0 is never emitted, with thr <= 0 every pick is.
 *                        shown_idx (room for n) int32 ascending, *count (device int32) their number, or -1 if the kernel
 *                        found its own lists corrupted.  n <= 2^24 (MI_E_UNSUPPORTED above).
 *   mi_plot_thumbs       patches (N, C, b, b) fp32, idx (n_shown) int32.  Per pick of idx: mean and population deviation
 *                        over all C b b values in double, q = rint(clip(255 ((x - mean) / std + 3) / 6, 0, 255)) in double
 *                        for every value (written to pre (n_shown, C, b, b) where pre is not null), then channel 0 of q
 *                        resized to T x T as torch's bilinear interpolation without align_corners and without antialias
 *                        does in float32, rounded half to even: out (n_shown, T, T) uint8.  A patch whose deviation is not
 *                        > 0, or an index outside [0, N), gives bytes 0.  b <= 192.
 *   mi_plot_patch_bytes  matplotlib's imsave(patch[0], cmap='gray'): per pick over channel 0, t = fl(fl(x - min) /
 *                        fl(max - min)) in float32, k = min(floor(256 t), 255), out (N, b, b) = lut256[k]; max == min
 *                        gives lut256[0].
 *   mi_plot_raster       a white (P, P, 3) uint8 canvas.  The map point (u, v) of shown pick k = y01[idx[k]] sits at column
 *                        M + rint(u S), row M + rint((1 - v) S), S = P - 1 - 2 M, in double.  mode 0: the discs
 *                        dx^2 + dy^2 <= R^2 of all shown picks in order, each in colours[idx[k]] (colours (N, 3)), then
 *                        all thumbnails (thumbs (n_shown, T, T) as grey, top-left at (column - T / 2, row - T / 2), inside a
 *                        1-pixel black frame) in order.  mode 1: thumbnail k, then the class box of labels[idx[k]]
 *                        (labels (N) int32 >= 0), for k in order; the box holds the decimal digits from glyphs (10, 7)
 *                        uint8 (7 rows of 5 bits, bit 4 the left pixel), each cell glyph_px square, glyph_gap between
 *                        digits, box_pad of white inside a box_border of (0, 0, 255) as the digits are; its bottom-left
 *                        pixel is (column - label_dx, row - label_dy).  Later primitives cover earlier ones; everything is
 *                        clipped at the canvas.  ws: mi_plot_raster_workspace_bytes(P), the priority image. */
typedef struct mi_plot_layout {
    int P, M, R, T, label_dx, label_dy, glyph_px, glyph_gap, box_pad, box_border;
} mi_plot_layout;
size_t mi_plot_select_workspace_bytes(long n, float thr);
int mi_plot_select(const float* y01, long n, float thr, int32_t* shown_idx, int32_t* count, void* ws, size_t ws_bytes,
                   mi_stream_t stream);
int mi_plot_thumbs(const float* patches, long N, int C, int b, const int32_t* idx, long n_shown, int T, uint8_t* out, uint8_t* pre,
                   mi_stream_t stream);
int mi_plot_patch_bytes(const float* patches, long N, int C, int b, const uint8_t* lut256, uint8_t* out, mi_stream_t stream);
size_t mi_plot_raster_workspace_bytes(int P);
int mi_plot_raster(const float* y01, long N, const int32_t* idx, long n_shown, const uint8_t* thumbs, const uint8_t* colours,
                   const int32_t* labels, const uint8_t* glyphs, const mi_plot_layout* layout, int mode, uint8_t* out, void* ws,
                   size_t ws_bytes, mi_stream_t stream);

/* The slice pictures of the detector's validation (`--debug 4`; reference trains/tomo_cr_semi_trainer.py:123-186 with
 * utils/debugger.py), DESIGN.md 4.19.  Volumes are row-major, addressed with 64-bit offsets.
 *   mi_dbgvis_minmax  vol (D, H, W) fp32, finite: out_minmax[2 i], [2 i + 1] = min, max of slice z0 + i, i < nz.  One
 *                     workgroup per slice; nz <= 65535.
 *   mi_dbgvis_render  tomo (D, H, W), hm_pred and hm_gt (D, h, w) fp32 with H == 2 h and W == 2 w (MI_E_ARG otherwise), minmax as
 *                     above for the same z0, nz.  out uint8 [4][nz][H][W][3], RGB, pictures pred_hm, gt_hm, pred_out, gt_out
 *                     of slice z = z0 + i:
 *                       grey     float32, every operation rounded: s = 1 / (mx - mn) (0 when mx == mn), t = (v - mn) s,
 *                                g = trunc(min(max(255 t, 0), 255)), three equal channels
 *                       up(m)    a = trunc(min(max(255 m, 0), 255)) in float32, then the 2 x bilinear enlargement with
 *                                half-pixel centres and replicated edges: (9 a00 + 3 a01 + 3 a10 + a11 + 8) >> 4, a00 the
 *                                nearest source pixel, the others its neighbours toward the output pixel's side
 *                       pred_hm  up(hm_pred), three equal channels
 *                       gt_hm    trunc(min(max(grey (1.0 - 0.7) + up(hm_gt) 0.7, 0), 255)) in float64
 *                       pred_out grey with, in (0, 0, 255), the ring of every pick with conf > conf_thresh and
 *                                (int)z_pick == z, centred at ((int)x, (int)y); gt_out the same for every centre of gt_dets
 *                                with (int)z == z.  A ring is the pixel set of the midpoint circle algorithm at `radius`
 *                                (0..31, MI_E_UNSUPPORTED above), clipped at the picture.
 *                     pred_dets (n_pred, 5) [x, y, z, score, conf] and gt_dets (n_gt, 3) [x, y, z] fp32 are HOST arrays in
 *                     picture coordinates: the entry builds the ring mask and the per-slice lists of centres on the host
 *                     and copies them into ws (mi_dbgvis_workspace_bytes(nz, n_pred, n_gt)) on the stream before the
 *                     launch.  Rows that are not finite are ignored.  nz <= 65535. */
int mi_dbgvis_minmax(const float* vol, int D, int H, int W, int z0, int nz, float* out_minmax, mi_stream_t stream);
size_t mi_dbgvis_workspace_bytes(int nz, long n_pred, long n_gt);
int mi_dbgvis_render(const float* tomo, const float* hm_pred, const float* hm_gt, int D, int H, int W, int h, int w, int z0,
                     int nz, const float* minmax, const float* pred_dets, long n_pred, const float* gt_dets, long n_gt,
                     float conf_thresh, int radius, uint8_t* out, void* ws, size_t ws_bytes, mi_stream_t stream);

/* Scoring the picks: the optimal matching of picks to target centres (reference evaluation/algorithms.py:6-21
 * `match_coordinates`, there a dense float64 matrix handed to scipy.optimize.linear_sum_assignment), DESIGN.md 4.21.
 *   mi_match_coordinates  preds (sumP, 3) and targets (sumT, 3) float64, the images of a split one after the other; image i
 *                         owns the rows [pred_off[i], pred_off[i + 1]) and [targ_off[i], targ_off[i + 1]).  pred_off and
 *                         targ_off (n_img + 1 each, ascending) are HOST arrays: the entry checks the sizes on the host and
 *                         copies both tables into the workspace on the stream before the launch.
 *                         Per image, in float64: d2[i][j] = |pred_i - target_j|^2, cost = min(d2 - radius^3, 0) (the CUBE of
 *                         the radius is the reference's), and the result is a rectangular assignment of minimum total cost
 *                         (shortest augmenting paths with dual variables: exact, no epsilon).  A pick counts as matched
 *                         only where its assigned cost is < 0: pred_to_target (sumP) = the target's index inside its image,
 *                         -1 otherwise; dist (sumP) = sqrt(d2) of the matched pair, 0 where unmatched; total_cost (n_img) =
 *                         the sum of the matched costs.  total_cost is unique; the assignment is not where sums tie (any
 *                         optimum may be returned, the same one for the same input).  The cost matrix is never stored.
 *                         One workgroup per image.  At most 4096 picks and 4096 targets per image: MI_E_UNSUPPORTED above,
 *                         returned before anything is enqueued - an input is never truncated.
 *   mi_match_workspace_bytes  for images of at most max_P picks and max_T targets; 0 beyond the limit.  Needs no device. */
size_t mi_match_workspace_bytes(int n_img, int max_P, int max_T);
int mi_match_coordinates(const double* preds, const double* targets, const int* pred_off, const int* targ_off, int n_img,
                         double radius, int* pred_to_target, double* dist, double* total_cost, void* workspace,
                         size_t workspace_bytes, mi_stream_t stream);

/* Grouping and tracing the picks: the detector's --spike and --fiber post-processing (reference utils/post_process.py:31-113
 * `tomo_group_postprocess`, `tomo_fiber_postprocess`; detectors/tomo_det_classify.py:196-216), DESIGN.md 4.23.
 * At most 4096 points per call: MI_E_UNSUPPORTED above, returned before anything is enqueued - an input is never truncated.
 * The source file is compiled with floating-point contraction off: d2, linspace and the Horner steps below are rounded
 * operation by operation, as numpy rounds them, and no fused multiply-add stands in for two of them.
 *   mi_pick_workspace_bytes  the scratch of both entries below for n points (the adjacency bit matrix, n x ceil(n / 64) words,
 *                            and the per-component fit table); 0 beyond the limit (and for n < 0).  Needs no device.
 *   mi_pick_components  pts (n, 3) float64.  i and j are joined where sqrt(d2) <= cutoff, d2 = (dx dx + dy dy) + dz dz in
 *                       float64, every product and sum rounded on its own: a pair at exactly the cutoff is decided as numpy
 *                       decides it.  label[i] = the smallest index of i's connected component, size[i] = its member count.
 *                       Two launches: the bit matrix by many workgroups, then one workgroup that merges labels in LDS with
 *                       integer atomics only - the same input gives the same bytes.  n == 0 is a no-op that returns MI_OK.
 *   mi_pick_fiber_fit   label, size as mi_pick_components wrote them for the same pts.  Column 0 of pts is the abscissa t,
 *                       columns 1 and 2 the ordinates u and v (the reference swaps columns 0 and 1 before it fits).  Every
 *                       component of MORE THAN 6 members, in ascending label order, members in index order:
 *                         lo, hi = min, max of t; span = hi - lo; m2 = int(span // 2), m_out = int(span // scale) (numpy's
 *                         floor_divide); a component with m2 == 0 is skipped (record written, not accepted, no rows).
 *                         u(t) and v(t) are fitted by a t^2 + b t + c in float64: least squares by the normal equations on
 *                         s = (t - (lo + hi) / 2) / (span / 2) and ordinates less their mean, solved twice (the second solve
 *                         fits the residual of the first), then carried back to powers of t.
 *                         res = (sum of squared residuals) / members.
 *                         k = max over y in linspace(lo - 1, hi + 1, m2) of 2 a / (1 + (2 a y + b)^2)^(2/3): the signed
 *                         maximum and the exponent 2/3 are the reference's.
 *                         accepted where, with tot = res_u + res_v: tot < res_cutoff and |k_u|, |k_v| < curvature_cutoff, or
 *                         res_cutoff <= tot < 3 res_cutoff and |k_u|, |k_v| < curvature_cutoff / 10.
 *                         An accepted component gives m_out rows [(int)y_j, (int)v_fit(y_j), (int)u_fit(y_j)], y =
 *                         linspace(lo - 1, hi + 1, m_out) exactly as numpy builds it (step = (stop - start) / (m_out - 1),
 *                         y_j = j step + start with the product and the sum rounded separately, the last element stop, a
 *                         single element start), the fits by Horner (a y + b) y + c, each step rounded, (int) toward zero.
 *                       THE ONE DIFFERENCE from the reference: a component whose t takes fewer than 3 distinct values gets
 *                       res_u = res_v = 10000 (numpy's empty residual), zero coefficients and is never accepted; the
 *                       reference would accept it, on a minimum-norm fit, where 3 res_cutoff > 20000.
 *                       comp: one record of 16 doubles per component of more than 6 members, room for n / 7 records: label,
 *                       members, lo, hi, a_u, b_u, c_u, res_u, a_v, b_v, c_v, res_v, k_u, k_v, accepted (0 / 1), rows written.
 *                       rows (cap_rows, 3) int32; *n_rows (device) = the total number of rows.  If they do not fit cap_rows
 *                       the entry writes none and returns MI_E_UNSUPPORTED, *n_rows the needed count.  The status depends
 *                       on that count, so this entry waits for the stream before it returns.  MI_E_ARG (*n_rows = -1) where
 *                       label / size describe more components than n / 7, or a component spans more than 2^24 in t. */
size_t mi_pick_workspace_bytes(int n);
int mi_pick_components(const double* pts, int n, double cutoff, int32_t* label, int32_t* size, void* ws, size_t ws_bytes,
                       mi_stream_t stream);
int mi_pick_fiber_fit(const double* pts, int n, const int32_t* label, const int32_t* size, double res_cutoff,
                      double curvature_cutoff, double scale, double* comp, int32_t* rows, int cap_rows, int32_t* n_rows, void* ws,
                      size_t ws_bytes, mi_stream_t stream);

/* The class gallery of plot_2d --class_gallery: per class the average patch, the spread of its members, their number and the
 * members nearest to their centroid, and the picture of all that (this project's own; nothing of it is in the reference),
 * DESIGN.md 4.24.  n <= 2^24 picks, k_classes <= 4096, 1 <= m <= 64, h w <= 2^20: MI_E_ARG outside, before anything is enqueued.
 * The kernels never read or write out of bounds for a label or an assignment outside its range (such a pick is in no class, such
 * an assignment is at distance +inf), but the counts then do not add up to n: the Python wrappers refuse both.
 * Both reductions first sort the picks by class on the device (histogram, exclusive scan, scatter in ascending pick index) and
 * add in that order with no floating-point atomic: the same input gives the same bytes.  The source file is compiled with
 * floating-point contraction off.
 *   mi_gallery_workspace_bytes  the scratch of mi_gallery_moments for patches of b = h w pixels, and of mi_gallery_exemplars
 *                         (which needs no more than b = 0); 0 outside the limits above.  Needs no device.
 *   mi_gallery_moments    patches (n, h, w) fp32, labels (n) int32.  count_out[c] = members of class c; mean_out[c], std_out[c]
 *                         (h, w) fp32 = the per-pixel mean and population deviation (divided by the count) of the members,
 *                         summed in float64 over the members in ascending pick index, 256 at a time into one partial sum each,
 *                         the partial sums added in order; the deviation in a second pass, sqrt(sum (x - mean)^2 / count) with
 *                         the float64 mean.  A class without members: count 0, mean and deviation 0.
 *   mi_gallery_exemplars  emb (n, dim) fp32, centroids (k_centroids, dim) fp32, assign (n) int32.  d2(i) = sum_j (emb[i][j] -
 *                         centroids[assign[i]][j])^2 in float64, j ascending, every difference, product and sum rounded on its
 *                         own.  idx_out (k_classes, m) int32: the m members of every class with the smallest d2, ascending by
 *                         (d2, pick index), -1 where the class has fewer; d2_out (k_classes, m) float64 their d2, +inf there.
 *                         A NaN distance counts as +inf.
 *   mi_gallery_raster     out_rgb (H, W, 3) uint8, white.  Row r shows class order_out[r]: descending count, ascending class
 *                         among equal counts (order_out (k_classes) int32 is written).  With PAD = 4 and the 5 x 7 digits of
 *                         glyphs (10, 7) uint8 drawn 2 pixels per bit, 2 pixels apart, in black: rows are max(h scale, 32) high
 *                         and start at y = 4 + r (row height + 4); the class number stands at x = 4 at the top of the row, the
 *                         count 18 pixels below it; the cells, h scale x w scale pixels each, start at x = 102 + j (w scale + 4):
 *                         j = 0 the mean, j = 1 the deviation, j = 2 + e exemplar e < m_show <= m of idx (k_classes, m) - a row
 *                         of patches (n, h, w); an idx outside [0, n) leaves the cell white.  H = 4 + k_classes (row height + 4),
 *                         W = 102 + (2 + m_show)(w scale + 4): MI_E_ARG for another canvas.  Source pixel (y / scale, x / scale).
 *                         Grey byte, all in float32, every operation rounded: span = max - min of the patch; 0 where span is
 *                         not positive, else rint(((v - min) / span) 255) (half to even), held in 0..255.  The deviation cell
 *                         takes min = 0 and span = the largest deviation of all classes and pixels.
 *   mi_gallery_raster_workspace_bytes  its scratch (the extremes of every cell); 0 outside the limits.  Needs no device. */
size_t mi_gallery_workspace_bytes(long n, int k_classes, int b, int m);
int mi_gallery_moments(const float* patches, const int32_t* labels, long n, int h, int w, int k_classes, float* mean_out,
                       float* std_out, int32_t* count_out, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_gallery_exemplars(const float* emb, const float* centroids, const int32_t* assign, const int32_t* labels, long n, int dim,
                         int k_centroids, int k_classes, int m, int32_t* idx_out, double* d2_out, void* ws, size_t ws_bytes,
                         mi_stream_t stream);
size_t mi_gallery_raster_workspace_bytes(int k_classes, int m_show);
int mi_gallery_raster(const float* mean, const float* std, const int32_t* count, const int32_t* idx, const float* patches, long n,
                      int h, int w, int k_classes, int m, int m_show, int scale, const uint8_t* glyphs, int32_t* order_out,
                      uint8_t* out_rgb, int H, int W, void* ws, size_t ws_bytes, mi_stream_t stream);

/* The SCAN step on stored embeddings, head-only form (the reference's SCANLoss and entropy, models/loss.py:68-119, summed over the
 * heads as its TomoSCANLoss does), DESIGN.md 4.25.  Logits are (B, H C) fp32, contiguous; head h owns columns h C .. h C + C - 1.
 * 1 <= C <= 64, 1 <= H <= 16, 1 <= B <= 65536 for the loss: MI_E_ARG outside, before anything is enqueued.  Per head, with
 * p = softmax(anchor row), q = softmax(neighbour row) (max-subtracted), s_i = p_i . q_i, m = (1 / B) sum_i p_i, x = max(m, 1e-8):
 *   consistency = -(1 / B) sum_i max(log s_i, -100)      entropy = -sum_c x_c log x_c      total = consistency - entropy_weight entropy
 * After the fp32 row maximum the arithmetic is float64; results are rounded to fp32 where they are stored.  No floating-point
 * atomic: the same input gives the same bytes.
 *   mi_scan_loss_workspace_bytes  the scratch of mi_scan_loss_fwd; 0 outside the limits.  Needs no device.
 *   mi_scan_loss_fwd    stats_out (H, 3) fp32 = total, consistency, entropy per head; *loss_out = the sum of the totals, heads in
 *                       ascending order; mean_out (H, C) float64 = m, kept for the backward pass.  Two launches: workgroup
 *                       (chunk, head) sums p and the clamped logs over MI_SCAN_CHUNK rows, then one workgroup adds the chunks in
 *                       ascending order and finishes every head.
 *   mi_scan_loss_bwd    d_anchors, d_neighbours (B, H C) fp32 = *dloss (device) times the gradient of *loss_out, one launch:
 *                       d total / d s_i = (s_i - 1) / max((1 - s_i) s_i, 1e-12) / B (0 at s = 1, finite at s = 0; the -100 clamp
 *                       passes no gradient test: torch's BCELoss), d total / d m_c = entropy_weight (log m_c + 1) where
 *                       m_c >= 1e-8, else 0, d m_c / d p_ic = 1 / B, and dz = p (g - p . g) through each softmax.
 *   mi_scan_assign      logits (n, H C) for any n >= 1: class_out (n, H) int32 = the argmax of the row's logits of head h, the
 *                       lowest index on an exact tie (0 for a row of NaNs); conf_out (n, H) fp32 its probability; prob_out
 *                       (n, H C) fp32 every probability, or NULL; counts_out (H, C) int32 the rows per class (integer atomics). */
#define MI_SCAN_CHUNK 256
size_t mi_scan_loss_workspace_bytes(int B, int C, int H);
int mi_scan_loss_fwd(const float* anchors, const float* neighbours, int B, int C, int H, double entropy_weight, float* stats_out,
                     float* loss_out, double* mean_out, void* ws, size_t ws_bytes, mi_stream_t stream);
int mi_scan_loss_bwd(const float* anchors, const float* neighbours, int B, int C, int H, double entropy_weight, const double* mean,
                     const float* dloss, float* d_anchors, float* d_neighbours, mi_stream_t stream);
int mi_scan_assign(const float* logits, long n, int C, int H, int32_t* class_out, float* conf_out, float* prob_out,
                   int32_t* counts_out, mi_stream_t stream);

/* After SCAN's clustering step (csrc/scan_selflabel.hip): the heads scored over the whole neighbour graph (the
 * reference's scan_evaluate, trains/eval_utils.py) and the self-labelling loss (ConfidenceBasedCE with MaskedCrossEntropyLoss,
 * models/loss.py:15-66).  Layout, limits on C and H, float64 after the fp32 row maximum and the fixed order of every sum are those
 * of the entries above: no floating-point atomic, the same input gives the same bytes.  MI_E_ARG outside the limits, before anything
 * is enqueued; the *_workspace_bytes functions need no device and return 0 outside the limits.
 *   mi_scan_graph_eval  logits (N, H C), 1 <= N < 2^31; index (N, k) int32, 1 <= k <= 64, entries in 0..N-1 (NOT checked on the
 *                       device: the caller validates the table); with_self != 0 makes the pick itself one more table entry, in
 *                       front, so K = k + 1, else K = k.  stats_out (H, 3) fp32 = total, consistency, entropy per head with
 *                         consistency = -(1 / (N K)) sum_i sum_j max(log(p_i . p_j), -100)   over the K entries j of row i
 *                         entropy = -sum_c x_c log x_c, x = max((1 / N) sum_i p_i, 1e-8)       total = consistency - entropy
 *                       (weight 1, as scan_evaluate); *best_out int32 = the head with the lowest total, the lowest index on an
 *                       exact tie.  Three launches: the float64 probabilities of every row into the workspace (N H C doubles) with
 *                       their sums per chunk of MI_SCAN_CHUNK rows; the pairs, a neighbour's probabilities read from the workspace;
 *                       one workgroup that adds the chunks in ascending order and finishes every head.
 *   mi_scan_selflabel_fwd  one head: weak, strong (B, C) fp32, 1 <= B <= 65536.  Per row p = softmax(weak), target = its argmax
 *                       (the lowest index on a tie), mask = max p > threshold compared in float64; n = masked rows, count_c = masked
 *                       rows with target c; w_c = 1 / (count_c / n), formed in fp32 with two correctly rounded divisions, where
 *                       balance != 0 and count_c > 0, else 1;
 *                         loss = sum_masked w_t (-log softmax(strong)_t) / sum_masked w_t   (F.cross_entropy's weighted mean)
 *                       loss_out fp32; info_out (3,) int32 = n, classes present, B; count_out (C,) int32; target_out (B,) int32;
 *                       mask_out (B,) uint8; *denom_out float64 = sum_masked w_t for the backward pass.  n = 0: loss 0, denom 0,
 *                       nothing divided.  Three launches: targets, mask and counts (integer atomics); the weighted sums per chunk;
 *                       one wave that adds the chunks in ascending order.
 *   mi_scan_selflabel_bwd  d_strong (B, C) fp32 = *dloss (device) mask_i w_t / denom (softmax(strong_i) - onehot(t_i)), one launch;
 *                       zeros for n = 0.  The weak logits get no gradient: target and mask are not differentiable. */
size_t mi_scan_graph_eval_workspace_bytes(long N, int C, int H);
int mi_scan_graph_eval(const float* logits, long N, int C, int H, const int32_t* index, int k, int with_self, float* stats_out,
                       int32_t* best_out, void* ws, size_t ws_bytes, mi_stream_t stream);
size_t mi_scan_selflabel_workspace_bytes(int B, int C);
int mi_scan_selflabel_fwd(const float* weak, const float* strong, int B, int C, double threshold, int balance, float* loss_out,
                          int32_t* info_out, int32_t* count_out, int32_t* target_out, uint8_t* mask_out, double* denom_out, void* ws,
                          size_t ws_bytes, mi_stream_t stream);
int mi_scan_selflabel_bwd(const float* strong, int B, int C, int balance, const int32_t* info, const int32_t* count,
                          const int32_t* target, const uint8_t* mask, const double* denom, const float* dloss, float* d_strong,
                          mi_stream_t stream);

/* How good a clustering of the picks is (csrc/cluster_quality.hip).  The reference has no counterpart (it judges
 * classes by eye in an interactive session); what is restated is scikit-learn's sklearn.metrics.silhouette_samples (Euclidean
 * metric), silhouette_score and contingency_matrix.  No allocation, no synchronisation, no floating-point atomic, every sum in a
 * fixed order: the same input gives the same bytes.  Rows and table entries are addressed with 64-bit offsets (the (n, k) float64
 * table passes 2 GiB near n = 10^6 at k = 256).  MI_E_UNSUPPORTED outside the limits, before anything is enqueued; the
 * *_workspace_bytes functions need no device and return 0 outside the limits.
 *   mi_silhouette_sums  x (n, d) fp32 rows, 2 <= n < 2^31, 1 <= d <= 512 (the limits of mi_knn_search); labels (n,) int32 fine
 *                       labels in [0, k), 1 <= k <= 1024; order (n,) int32 = the picks sorted by label, picks of one label in
 *                       ascending index (a stable sort; the caller's plumbing).  sums_out (n, k) float64:
 *                         sums_out[i][c] = sum over the members j != i of fine cluster c of sqrt(max(d2(i, j), 0))
 *                       d2(i, j) = |x_i|^2 + (|x_j|^2 - 2 x_i.x_j) in fp32, the bytes of mi_knn_search's MI_KNN_L2 value before its
 *                       clamp (the row-product tile of rowdot.h, bf16x3 on the matrix cores); the pair (i, i) is left out by
 *                       index; the square root and every sum are float64.  The n x n distances are never stored.  Columns are
 *                       laid out cluster by cluster, each cluster padded to whole tiles of 32 columns; a wave takes 64 rows (32
 *                       where the rows' cut passes 160 KB of LDS) against one chunk of a cluster's tiles (chunks of
 *                       max(32, ceil((n / 32 + k) / 64)) tiles), adds a lane's column over the chunk's tiles in ascending order,
 *                       then the 32 lanes in a fixed tree; a last launch adds a cluster's chunks in ascending order.  A label
 *                       outside [0, k), or an order that is not that sort, is NOT detected (the caller validates): such picks
 *                       are left out of every sum, never read or written out of bounds.
 *   mi_silhouette_finalise  sums (n, k) float64 as above, labels as above, class_of (k,) int32 in [0, C), 2 <= C <= 1024 (the
 *                       identity when nothing is merged).  A class's sum is the sum of its fine clusters' columns in ascending
 *                       fine index, its count the integer sum of theirs.  Per pick, float64: a = own-class sum / (count - 1),
 *                       b = min over the other non-empty classes of sum / count, s = (b - a) / max(a, b) (0 where that is 0 / 0);
 *                       a = s = 0 for the only member of its class (as sklearn); nearest_out int32 = the class attaining b, the
 *                       lowest index on a tie.  class_count_out (C,) int32; class_mean_out (C,) float64 = mean of s over the
 *                       class, NaN for a class without members; *mean_out = mean of s over all picks (per chunk of 256 picks the
 *                       sum in pick order, the chunks in ascending order); confusion_out (C, C) int32 [own][nearest] (integer
 *                       atomics).  info_out (3,) int32 = non-empty classes, the largest class count, status: 0 ok, 1 fewer than
 *                       two non-empty classes or every class a singleton, 2 a class_of entry outside [0, C).  With a status
 *                       other than 0 only info_out and class_count_out are written: the caller reads info_out and raises.
 *   mi_label_contingency  a, b (n,) int32, labels outside [0, ca) x [0, cb) left out; table_out (ca, cb) int64 counts (integer
 *                       atomics), 1 <= ca, cb and ca cb <= 2^24. */
size_t mi_silhouette_workspace_bytes(long n, int d, int k);
int mi_silhouette_sums(const float* x, const int32_t* labels, const int32_t* order, long n, int d, int k, double* sums_out, void* ws,
                       size_t ws_bytes, mi_stream_t stream);
size_t mi_silhouette_finalise_workspace_bytes(long n, int k, int C);
int mi_silhouette_finalise(const double* sums, const int32_t* labels, const int32_t* class_of, long n, int k, int C, double* s_out,
                           double* a_out, double* b_out, int32_t* nearest_out, double* class_mean_out, int32_t* class_count_out,
                           double* mean_out, int32_t* confusion_out, int32_t* info_out, void* ws, size_t ws_bytes,
                           mi_stream_t stream);
int mi_label_contingency(const int32_t* a, const int32_t* b, long n, int ca, int cb, int64_t* table_out, mi_stream_t stream);

/* Label spreading over the neighbour graph (csrc/label_spread.hip): Zhou et al. 2004, "Learning with local and
 * global consistency", as scikit-learn's LabelSpreading states it.  The reference gets from a few examples to all similar picks by
 * hand in its interactive session.  The graph is index (n, k) int32 with its transpose rev_ptr (n + 1), rev_edge (n k) as
 * csrc/knn_graph.h describes them (n k < 2^31; MI_E_UNSUPPORTED outside, before anything is enqueued); damaged entries are passed
 * over by that header's guards.  No allocation, no synchronisation, no floating-point atomic, every sum in an order the graph
 * fixes: the same input gives the same bytes.
 *   mi_spread_weights    dist (n, k) fp32 squared L2 as mi_knn_search writes it.  w_out (n, k) fp32, 0 for an edge that is passed
 *                        over.  mode 0: 1 for every valid edge (dist and scale_out may be NULL).  mode 1: the self-tuning Gaussian
 *                        of Zelnik-Manor & Perona, w_ij = exp(-d2_ij / sqrt(s_i s_j)) in fp32 with sqrt(s_i s_j) formed as
 *                        sqrt(s_i) sqrt(s_j); s_i = scale_out[i] = the largest finite dist of row i (0 where there is none); where
 *                        s_i s_j = 0, w = 1 if d2 = 0, else 0; a d2 that is not finite gives 0.
 *   mi_spread_csr_count  a wave per vertex walks its incident list: the valid forward edges in column order, then the edges of its
 *                        reverse range that have no opposite edge, in range order.  count_out (n,) int64 = entries of the vertex;
 *                        deg_out (n,) float64 = the sum of w_sym(i, j) = max(w_ij, w_ji), an absent direction 0, over the list (64
 *                        entries in one fixed tree, the batches in list order).  The caller's exclusive scan of count_out is
 *                        row_ptr (n + 1) int64.
 *   mi_spread_csr_fill   the same walk: col_out (nnz,) int32 and val_out (nnz,) float64 = w_sym (dis_i dis_j), dis = 1 / sqrt(deg)
 *                        and 0 where deg = 0; dis_i dis_j is formed first, so the matrix is symmetric to the bit.  nnz =
 *                        row_ptr[n]; nothing is written outside [row_ptr[i], row_ptr[i + 1]) or [0, nnz).
 *   mi_spread_step       F_out[i, :] = alpha sum_e val_e F_in[col_e, :] + (1 - alpha) Y[i, :] over the entries e of row i in
 *                        order; F_in, Y, F_out (n, C) float64 row-major, 2 <= C <= 64 (MI_E_UNSUPPORTED outside, before anything is
 *                        enqueued), 0 < alpha < 1 and F_out overlapping neither input (MI_E_ARG).  col must lie in [0, n): the
 *                        CSR of the two entries above does.  residual_out, where not NULL, is one 64-bit device word that
 *                        receives max |F_out - F_in| as the bits of that non-negative double (zeroed by the entry, then an integer
 *                        atomicMax per workgroup); NULL skips it.
 *   mi_spread_decide     label_out int32 = argmax_c F[i, c], ties to the lowest c; mass_out = sum_c F[i, c] in ascending c;
 *                        conf_out = F[i, label] / mass (0 where the mass is 0); label -1 where the mass is 0 or conf < min_conf.
 *   mi_seed_nearest      picks (n, 3), seeds (m, 3) float64 with pick_tomo (n,), seed_tomo (m,) int32.  One workgroup per seed:
 *                        pick_out[s] int32 = the pick of the seed's tomogram with the least (dx dx + dy dy) + dz dz (float64,
 *                        no contraction), ties to the lowest pick; -1 where its distance exceeds radius or the tomogram has no
 *                        pick; dist_out[s] = that least distance (+inf without a pick).  No limit on n or m below 2^31. */
int mi_spread_weights(const int32_t* index, const float* dist, long n, int k, int mode, float* scale_out, float* w_out,
                      mi_stream_t stream);
int mi_spread_csr_count(const int32_t* index, const int32_t* rev_ptr, const int32_t* rev_edge, const float* w, long n, int k,
                        int64_t* count_out, double* deg_out, mi_stream_t stream);
int mi_spread_csr_fill(const int32_t* index, const int32_t* rev_ptr, const int32_t* rev_edge, const float* w, long n, int k,
                       const int64_t* row_ptr, const double* deg, long nnz, int32_t* col_out, double* val_out, mi_stream_t stream);
int mi_spread_step(const int64_t* row_ptr, const int32_t* col, const double* val, long n, int C, double alpha, const double* F_in,
                   const double* Y, double* F_out, uint64_t* residual_out, mi_stream_t stream);
int mi_spread_decide(const double* F, long n, int C, double min_conf, int32_t* label_out, double* conf_out, double* mass_out,
                     mi_stream_t stream);
int mi_seed_nearest(const double* picks, const int32_t* pick_tomo, long n, const double* seeds, const int32_t* seed_tomo, long m,
                    double radius, int32_t* pick_out, double* dist_out, mi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CETPICK_HIP_H */
