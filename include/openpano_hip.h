/* include/openpano_hip.h -- C-ABI of libopenpano_hip.so, the MI355X (gfx950) implementation of
 * OpenPano's data-parallel hot path.
 *
 * The reference has no FFI: its seam is the C++ class surface.  Each entry point below names
 * the reference interface it stands in for (file:line under /root/reference/src); the C++
 * adapters in openpano_amd/host/pano_hip.hh re-expose the reference's own class names
 * (FeatureDetector::detect_feature, PairWiseMatcher::match, ...) on top of these calls, and
 * INTEGRATION.md shows the binding a maintainer would add to the reference tree.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch types cross this boundary;
 *   - every function returns OP_OK (0) or a negative op_status; op_last_error() gives the
 *     message of the calling thread's last failure (the adapters turn it into the reference's
 *     error_exit(), lib/debugutils.cc:57-60); no exception crosses the ABI;
 *   - images are the reference's Mat32f layout (lib/mat.h:8-57): row-major H x W x 3 fp32 in
 *     [0,1], or the decoder's bytes in the same layout (OP_U8 / OP_SRC_U8), read as (float)byte / 255.0 like read_img
 *     does; a pointer may be host or device memory (flag on_device);
 *   - there is NO CPU fallback: without a gfx950 device every compute entry point fails.
 */
#ifndef OPENPANO_HIP_H
#define OPENPANO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
	OP_OK = 0,
	OP_ERR_INVALID = -1,      /* bad argument */
	OP_ERR_HIP = -2,          /* a HIP runtime call failed (message has the hipError string) */
	OP_ERR_CAPACITY = -3,     /* a device-side work list overflowed its capacity */
	OP_ERR_UNSUPPORTED = -4,  /* configuration outside what the kernels implement */
	OP_ERR_NO_FEATURE = -5    /* an image produced zero features (stitcherbase.cc:20-21) */
} op_status;

const char* op_last_error(void);
/* library/ABI version, bumped on incompatible change */
int op_abi_version(void);

/* ---- configuration: POD snapshot of namespace config (lib/config.hh:24-85), taken by the
 * adapters at every call because the CLI fills the globals after static init (main.cc:237-292) */
typedef struct op_config {
	/* SIFT (config.cfg:19-41) */
	int SIFT_WORKING_SIZE, NUM_OCTAVE, NUM_SCALE;
	float SCALE_FACTOR, GAUSS_SIGMA;
	int GAUSS_WINDOW_FACTOR;
	float JUDGE_EXTREMA_DIFF_THRES, CONTRAST_THRES, PRE_COLOR_THRES, EDGE_RATIO;
	int CALC_OFFSET_DEPTH;
	float OFFSET_THRES;
	float ORI_RADIUS;
	int ORI_HIST_SMOOTH_COUNT;
	int DESC_HIST_SCALE_FACTOR, DESC_INT_FACTOR;
	/* matching / RANSAC (config.cfg:45-54) */
	float MATCH_REJECT_NEXT_RATIO;
	int RANSAC_ITERATIONS;
	double RANSAC_INLIER_THRES;
	float INLIER_IN_MATCH_RATIO, INLIER_IN_POINTS_RATIO;
	/* modes that change kernel behaviour (config.cfg:2-10,69) */
	int CYLINDER, TRANS, ESTIMATE_CAMERA, ORDERED_INPUT, LAZY_READ, MULTIBAND;
	int MAX_OUTPUT_SIZE;
	float FOCAL_LENGTH;
} op_config;
/* shipped defaults, src/config.cfg */
void op_config_default(op_config* cfg);

/* ---- context: one per (process, device); owns the stream and the HBM workspaces.
 * stream = NULL creates a private hipStream; otherwise the caller's hipStream_t is used (e.g.
 * torch.cuda.current_stream().cuda_stream) and all work is ordered on it. Thread-compatible:
 * concurrent calls need distinct contexts (StitcherBase::calc_feature's omp loop,
 * stitcherbase.cc:14, maps to ONE batched call instead). */
typedef struct op_ctx op_ctx;
int op_ctx_create(int device, void* hip_stream, op_ctx** out);
void op_ctx_destroy(op_ctx* ctx);
int op_ctx_sync(op_ctx* ctx);
/* Per-stage device timing with HIP events on the context's stream -- the counterpart of the
 * reference's TotalTimer table (lib/timer.hh:63-83, dumped at exit by main.cc:336); stage labels
 * reuse the reference's ("build pyramid", "extrema", "sift descriptor", "matcher", ...). */
int op_ctx_set_profiling(op_ctx* ctx, int enable);
/* Restrict the timing to ONE stage label (NULL or "": all stages).  Every bracketed stage costs two event records and
 * the gap they put between kernels (measured: 0.05 ms on the 1.05 ms SIFT step with five stages bracketed); a caller
 * that times its own loop and wants one kernel's duration from inside it brackets that kernel only. */
int op_ctx_profile_only(op_ctx* ctx, const char* label);
int op_ctx_profile_reset(op_ctx* ctx);
int op_ctx_profile_count(op_ctx* ctx);
int op_ctx_profile_get(op_ctx* ctx, int i, const char** label, double* total_ms, long* calls);

typedef struct op_image {
	const void* data;    /* H x W x 3, row-major interleaved RGB; element type per dtype */
	int h, w;
	int on_device;       /* 0: host pointer (copied H2D inside the call), 1: device pointer.  Host images of a batch that lie at
	                      * one constant stride >= their size (a contiguous array of frames, a decoder pool) go up in ONE copy;
	                      * pinned memory copies at the link rate */
	int dtype;           /* OP_F32 (0): fp32 in [0,1] = Mat32f ; OP_U8 (1): decoder bytes, converted on the
	                      * device exactly like read_img does, (float)byte / 255.0 (lib/imgio.cc:54-56,75-77):
	                      * a quarter of the PCIe / HBM traffic of the fp32 image */
} op_image;
enum { OP_F32 = 0, OP_U8 = 1 };

/* =====================================================================================
 * SIFT  -- replaces FeatureDetector::detect_feature / SIFTDetector::do_detect_feature
 * (feature/feature.hh:50-57, feature/feature.cc:20-47) looped over images by
 * StitcherBase::calc_feature (stitch/stitcherbase.cc:9-27).
 * One call extracts the features of n images; results stay resident in HBM inside an
 * op_features object so that the matcher reads them without a second H2D pass.
 * Output order per image is canonical: sorted by (octave, scale, y, x, real_x, real_y) of the
 * refined keypoint, then orientation-peak order (the reference's order is thread-timing
 * dependent, feature/extrema.cc:56).
 * ===================================================================================== */
typedef struct op_features op_features;
int op_sift_batch(op_ctx* ctx, const op_config* cfg, const op_image* imgs, int n, op_features** out);
/* The same for HOST images with the transfers overlapped (StitcherBase::calc_feature end to end, stitch/stitcherbase.cc:9-27:
 * Mat32f / decoder bytes in host memory in, descriptors and keypoint coordinates in host memory out).  The batch runs as
 * a pipeline over chunks: uploads on one copy stream, kernels on the context's stream, results on a second copy stream
 * into desc_out (rows x 128 fp32) / coor_out (rows x 2 fp64), images back to back, capacity_rows rows of room (either
 * pointer may be NULL; pinned memory copies at the link rate).  *out receives the resident features as op_sift_batch
 * does.  OP_ERR_CAPACITY (with *out still set) when the host buffers are too small. */
int op_sift_batch_host(op_ctx* ctx, const op_config* cfg, const op_image* imgs, int n,
		float* desc_out, double* coor_out, int64_t capacity_rows, op_features** out);
int op_features_num_images(const op_features* f);
/* number of descriptors of image i (K_i) and the exclusive prefix offset of its first row */
int op_features_count(const op_features* f, int i);
int64_t op_features_offset(const op_features* f, int i);
int64_t op_features_total(const op_features* f);
/* device-resident flat buffers: desc = total x 128 fp32, coor = total x 2 fp64
 * (coordinates relative to the image centre in original-image pixels, feature.cc:23-26) */
const float* op_features_desc_device(const op_features* f);
const double* op_features_coor_device(const op_features* f);
/* D2H copy of image i's K_i x 128 descriptors and K_i x 2 coordinates (either may be NULL) */
int op_features_copy(op_ctx* ctx, const op_features* f, int i, float* desc, double* coor);
/* D2H copy of image i's K_i x 2 real_coor in [0,1) -- what SIFTDetector::do_detect_feature itself
 * returns (feature/feature.cc:31-47) before FeatureDetector::detect_feature re-centres it (:20-28);
 * the C++ adapter's do_detect_feature override hands these to the reference's base class */
int op_features_copy_real(op_ctx* ctx, const op_features* f, int i, double* real);
/* build an op_features from host arrays (debug commands / tests: match without SIFT).
 * desc may be NULL (coordinates only: enough for op_ransac_pairs; op_match_pairs then fails) */
int op_features_from_host(op_ctx* ctx, const float* const* desc, const double* const* coor,
		const int* counts, int n, op_features** out);
/* the same from a flat DEVICE buffer (images back to back; D2D copy) -- the multi-GPU path hands
 * the all-gathered descriptors of every rank's images to the matcher this way */
int op_features_from_device(op_ctx* ctx, const float* desc_dev, const double* coor_dev,
		const int* counts, int n, op_features** out);
/* the same without the copy: the table ADOPTS the caller's device buffers (total x 128 fp32, total x 2 fp64, images
 * back to back), which must stay valid and unchanged until op_features_free -- the exchange step of the multi-GPU
 * path receives every rank's features straight into such a table and hands it to the matcher as it is */
int op_features_adopt_device(op_ctx* ctx, const float* desc_dev, const double* coor_dev,
		const int* counts, int n, op_features** out);
void op_features_free(op_features* f);

/* Staged single-image run keeping every intermediate (the debug commands raw_extrema /
 * keypoint / orientation of main.cc:41-81 and the per-stage parity tests).
 * plane kinds: 1 DoG[s] (s in 0..nscale-2), 2 mag[s], 3 ort[s] (s in 1..nscale-3),
 *              4 working RGB, 5 grey octave base, 6 Gaussian[s] (s in 1..nscale-1).
 * Only the Gaussian stack reaches HBM in op_sift_batch: DoG planes live in LDS for the extrema scan and are
 * re-evaluated as |G[s] - G[s+1]| (feature/dog.cc:126) where the refinement needs them; mag/ort are evaluated
 * by the orientation / descriptor kernels (GaussianPyramid::cal_mag_ort, feature/dog.cc:60-94) on the Gaussian
 * plane for the samples they use.  The dump computes DoG, mag and ort planes on request. */
typedef struct op_sift_dump op_sift_dump;
int op_sift_staged(op_ctx* ctx, const op_config* cfg, const op_image* img, op_sift_dump** out);
void op_sift_dump_free(op_sift_dump* d);
int op_sift_dump_working_dims(const op_sift_dump* d, int* h, int* w);
int op_sift_dump_octave_dims(const op_sift_dump* d, int oct, int* h, int* w);
int op_sift_dump_plane(op_ctx* ctx, const op_sift_dump* d, int kind, int oct, int s, float* out);
int op_sift_dump_raw_count(const op_sift_dump* d, int oct, int s);
int op_sift_dump_raw(const op_sift_dump* d, int oct, int s, int* xy);       /* sorted (y, x) */
/* which: 0 refined, 1 oriented; ints = x,y,octave,scale; real = real_coor; fl = dir, scale_factor */
int op_sift_dump_kp_count(const op_sift_dump* d, int which);
int op_sift_dump_kp(const op_sift_dump* d, int which, int* ints, double* real, float* fl);
int op_sift_dump_desc(const op_sift_dump* d, float* desc, double* coor);    /* coor in [0,1) */

/* device math twins of glibc expf/cosf/sinf/hypotf and of fast_atan (feature/dog.cc:22-37),
 * evaluated on the GPU over n host values (tests: device == reference libm, bit for bit).
 * which: 0 expf(x), 1 cosf(x), 2 sinf(x), 3 hypotf(x,y), 4 fast_atan(y,x)+pi */
int op_debug_math(op_ctx* ctx, int which, const float* x, const float* y, int n, float* out);
/* Per-image capacity of the context's raw / refined candidate lists (default 16384).  The lists
 * are speculative: a batch that outgrows them re-runs once with the observed size and the context
 * keeps the larger capacity (the reference appends to std::vectors, extrema.cc:36-61).  Exposed so
 * that tests can force the overflow path with a tiny capacity; >= 64. */
int op_debug_set_raw_capacity(op_ctx* ctx, int cap);
/* Floats of LDS list arena one sorting pass of the descriptor kernel may use (default and maximum 640).  A batch of 64
 * window samples (sift.cc:110-146) whose per-bin lists, padded to float4s, need more is sorted and accumulated in two
 * passes of 32 samples; exposed so that tests can force that path (0: always). */
int op_debug_set_desc_list_cap(op_ctx* ctx, int floats);
/* The process-wide device pool, read under its lock: blocks handed out and not yet returned, their bytes (size
 * classes), and the bytes of returned blocks the pool keeps for reuse.  Any pointer may be NULL.  Exposed so that tests
 * can check that every call gives back what it took, on refusals as well. */
int op_debug_pool_stats(int64_t* live_blocks, int64_t* live_bytes, int64_t* cached_bytes);
/* Rows the last op_match_pairs call on ctx that swept anything queued for the exact full scan, forward and reverse
 * (-1 each before the first such call; a refused call counts: the numbers are what its message reports).  The next call
 * sizes its exact-scan launches from them.  Either pointer may be NULL.  Read-only; exposed so that tests can check that a
 * scene queued the rows it was built to queue. */
int op_debug_match_last_slow(op_ctx* ctx, int* forward_rows, int* reverse_rows);

/* =====================================================================================
 * MATCH -- replaces PairWiseMatcher (feature/matcher.hh:40-67, matcher.cc:73-135) as used by
 * Stitcher::pairwise_match / linear_pairwise_match (stitch/stitcher.cc:96-136), with the
 * semantics of the reference's exact matcher FeatureMatcher::match (matcher.cc:15-71): 2-NN
 * ratio test from the smaller set, then the reverse test.  All requested pairs are
 * matched in one launch series; MFMA tiles (two-term bf16 split, fp32 accumulate) rank candidates, an exact re-score in the
 * reference's summation order (feature/dist.cc:22-57) decides.
 * ===================================================================================== */
typedef struct op_matches op_matches;
/* pairs: npairs x 2 image indices (i, j) into f.  The result stays in HBM -- per image pair a list of
 * <idx in image i, idx in image j> sorted by (first, second) (MatchData, matcher.hh:14-25), pairs back to back in
 * the order of `pairs` -- where op_ransac_pairs reads it; the call itself brings back the per-pair counts only.
 * An op_matches must not outlive the context it was made with. */
int op_match_pairs(op_ctx* ctx, const op_config* cfg, const op_features* f,
		const int* pairs, int npairs, op_matches** out);
int op_matches_count(const op_matches* m, int p);
/* the list of pair p on the host; the first copy fetches the whole job's lists from the device (one D2H),
 * later ones are lookups.  Thread-safe (PairWiseMatcher::match is called concurrently, stitcher.cc:106-109). */
int op_matches_copy(const op_matches* m, int p, int* idx_pairs);
/* every list at once: idx_pairs = total x 2 ints (may be NULL), offsets = npairs + 1 entries (may be NULL) */
int op_matches_copy_all(const op_matches* m, int* idx_pairs, int64_t* offsets);
/* the device-resident flat list (total x 2 int32), NULL when the lists were wrapped from host arrays */
const int* op_matches_device_list(const op_matches* m);
int64_t op_matches_total(const op_matches* m);
/* wrap host match lists (npairs lists of counts[p] <first, second> pairs): debug / test entry */
int op_matches_from_host(const int* const* idx_pairs, const int* counts, int npairs, op_matches** out);
/* a's pairs followed by b's as ONE result (both made with contexts of ctx's device): what a rank of a sharded job passes to
 * op_ransac_pairs when it matched its pair list in two calls (stitcher.cc:100-113 is one loop over all pairs).  The new
 * object owns a copy of the lists; a and b stay valid and are freed by the caller. */
int op_matches_concat(op_ctx* ctx, const op_matches* a, const op_matches* b, op_matches** out);
void op_matches_free(op_matches* m);

/* =====================================================================================
 * SEVERAL GPUs IN ONE PROCESS -- SURVEY 8(e): the reference's two parallel loops are the axes
 * (images: stitch/stitcherbase.cc:14-25; image pairs: stitch/stitcher.cc:96-113).  A group owns
 * one context (stream, workspaces, one host thread per call) per listed device.  The *_multi calls
 * return exactly what the single-device calls return; with one device they ARE those calls.
 * (One process per GPU with an RCCL all-gather instead: openpano_amd/distributed.py.)
 * ===================================================================================== */
typedef struct op_group op_group;
int op_group_create(const int* devices, int ndev, op_group** out);   /* a device may be listed twice */
void op_group_destroy(op_group* g);
int op_group_size(const op_group* g);
op_ctx* op_group_ctx(op_group* g, int k);                             /* context k; context 0 holds gathered results */
/* StitcherBase::calc_feature sharded by image: contiguous blocks of n / ndev images per context; the features are
 * all-gathered device-to-device over xGMI (every device pulls the other devices' slices over its own links) -- the
 * returned op_features is the table on context 0 and carries its replicas on the other devices.  Host images only,
 * or device images resident on the device of the context that owns them. */
int op_sift_batch_multi(op_group* g, const op_config* cfg, const op_image* imgs, int n, op_features** out);
/* Stitcher::pairwise_match sharded by pair: every device uses its replica of the table (made by op_sift_batch_multi, or
 * pulled from f's device on first use), the pair list is dealt balanced by K_i * K_j, each device keeps the lists of
 * its pairs resident; counts / lists read back in the order of `pairs`. */
int op_match_pairs_multi(op_group* g, const op_config* cfg, const op_features* f, const int* pairs, int npairs, op_matches** out);
/* TransformEstimation for the same job (stitch/stitcher.cc:66-94 inside the pair loop): every device estimates the pairs it
 * matched -- their match lists are resident there -- with the seeds op_ransac_pairs would give them; the result is in the
 * order of `pairs`.  m from op_match_pairs (one device) or wrapped host lists runs on context 0. */
struct op_ransac_result;
int op_ransac_pairs_multi(op_group* g, const op_config* cfg, const op_features* f, const op_matches* m,
		const int* pairs, int npairs, const int* shapes_wh, const uint32_t* seeds, uint32_t base_seed,
		struct op_ransac_result** out);

/* =====================================================================================
 * RANSAC -- replaces TransformEstimation(...).get_transform(MatchInfo*)
 * (stitch/transform_estimate.hh:22-31, transform_estimate.cc:26-218) for every pair at once.
 * pairs / m must be the pair list and result of op_match_pairs (match p belongs to pairs[p]);
 * keypoint coordinates come from f (centred original-image pixels); shapes_wh holds (w, h) of
 * every image of f (Shape2D, stitch/match_info.hh:53-78).  The matched point pairs are gathered on the
 * device from m's resident lists and f's coordinates (nothing is re-uploaded); one D2H brings back the
 * winners and the gathered points for the host-side acceptance gates of fill_inliers_to_matchinfo.
 * Homography (8-point samples) unless cfg->CYLINDER || cfg->TRANS (affine, 7-point samples).
 * Sampling is std::mt19937 with the reference's duplicate rejection; pair p is seeded with
 * seeds[p], or from base_seed and p when seeds == NULL (the reference seeds from
 * std::random_device, i.e. is not reproducible: transform_estimate.cc:64-65).
 * The result mirrors MatchInfo (stitch/match_info.hh:14-51): ok = get_transform()'s return,
 * confidence (negative = -#inliers, as the reference leaves it on rejection), homo (image j ->
 * image i), inlier indices into the pair's match list.
 * ===================================================================================== */
typedef struct op_ransac_result op_ransac_result;
int op_ransac_pairs(op_ctx* ctx, const op_config* cfg, const op_features* f, const op_matches* m,
		const int* pairs, int npairs, const int* shapes_wh, const uint32_t* seeds, uint32_t base_seed,
		op_ransac_result** out);
int op_ransac_ok(const op_ransac_result* r, int p);
float op_ransac_confidence(const op_ransac_result* r, int p);
int op_ransac_homo(const op_ransac_result* r, int p, double* h9);
int op_ransac_inlier_count(const op_ransac_result* r, int p);
int op_ransac_inliers(const op_ransac_result* r, int p, int* match_indices);
/* index of the winning hypothesis and its inlier count (-1: no healthy hypothesis) */
int op_ransac_best(const op_ransac_result* r, int p, int* hyp, int* count);
/* number of accepted pairs and the inliers they hold, over the whole result */
int op_ransac_summary(const op_ransac_result* r, int* accepted_pairs, int64_t* inliers);
void op_ransac_free(op_ransac_result* r);

/* Stitcher::match_image's bookkeeping for a whole job (stitch/stitcher.cc:79-93): every ACCEPTED pair (i, j) of the result
 * becomes two directed entries -- pairwise_matches[i][j] = MatchInfo{confidence, homo (j -> i), matches (point in i, point
 * in j)} and pairwise_matches[j][i] = the same with homo.inverse() scaled by 1 / inv[8] and every match reversed
 * (match_info.hh:21-25) -- in the flat form pano_estimate_cameras (include/pano_host.h) takes: CameraEstimator's input
 * without a pass through the caller's own containers.  `pairs` / npairs MUST be those of the op_ransac_pairs call that made r,
 * m the match lists it read (r keeps a hash of that pair list: another list is refused with OP_ERR_INVALID).  On any failure
 * the output arrays may be partly written.  Sizes first: entries = 2 x accepted pairs, points = total rows of pts.
 *   ij      entries x 2        conf  entries        homo  entries x 9        cnt  entries
 *   pts     points x 4 (first.x, first.y, second.x, second.y), entries back to back */
int op_pairwise_table_size(const op_ransac_result* r, int* entries, int64_t* points);
int op_pairwise_table(op_ctx* ctx, const op_features* f, const op_matches* m, const op_ransac_result* r, const int* pairs, int npairs,
		int* ij, float* conf, double* homo, int* cnt, double* pts);

/* =====================================================================================
 * WARP + BLEND -- replaces ConnectedImages::blend() (stitch/stitcher_image.hh:92,
 * stitch/stitcher_image.cc:116-155) together with the blender it constructs:
 * LinearBlender (stitch/blender.cc:24-96; cfg->MULTIBAND == 0, both cfg->LAZY_READ branches,
 * weights per cfg->ORDERED_INPUT) or MultiBandBlender(cfg->MULTIBAND) (stitch/multiband.cc:19-151).
 * BlenderBase::add_image takes the coordinate map as a std::function (stitch/blender.hh:52-56),
 * which a device cannot call, so the seam sits one level up and the map travels as PODs:
 * projection method, proj_range.min, resolution and homo_inv per image.
 * Pixels are the reference's, bit for bit, for every projection (the map's sin / cos / tan are tabulated per canvas
 * column / row by the host libm, colour arithmetic is the reference's fp32 sequence); Color::NO = -1 marks
 * "no pixel" on input and output (lib/color.cc:11-15).  "The host libm" is the one this library is linked against: the
 * claim is bit-for-bit against a reference built on the same glibc (sin / cos / tan of other libms may differ in the last place).
 * Threading: the tables are cached per context -- geometry key + host and device copy, (2 W + H) doubles each, for the
 * context's lifetime).  Like every other per-context workspace they make an op_ctx THREAD-COMPATIBLE, not thread-safe:
 * one call at a time per context; concurrent callers use one context each (as the adapters in pano_hip.hh do).
 * Multiband: a cfg->MULTIBAND / cfg->GAUSS_WINDOW_FACTOR whose blur at some level is wider than 31 taps (GaussCache's
 * half-width above 15: wf at levels 0-2, 1.5 wf at 3-8, 2 wf at 9) returns OP_ERR_UNSUPPORTED, before any device work.
 * ===================================================================================== */
enum { OP_SRC_DEVICE = 1, OP_SRC_U8 = 2 };   /* bits of op_blend_image.on_device */
typedef struct op_blend_image {
	const float* data;    /* H x W x 3 fp32 (ImageRef::img, stitch/imageref.hh:15-17); with OP_SRC_U8: H x W x 3 bytes behind the same pointer */
	int h, w;
	/* A flag word.  Bit 0, OP_SRC_DEVICE: data is a device pointer (0 and 1 mean what they always meant).  Bit 1, OP_SRC_U8:
	 * data points at mat_h x mat_w x 3 decoder bytes; a sample's four taps are converted on the device exactly like read_img
	 * does, (float)byte / 255.0 (lib/imgio.cc:55-57,78-80), then interpolated in the reference's fp32 sequence: the canvas
	 * and the overlap statistics equal, bit for bit, those of the fp32 view that conversion produces.  A byte view holds no
	 * Color::NO.  A host byte view uploads 3 h w bytes instead of 12 h w; a device byte view may lie at any alignment and
	 * only its own bytes are read.  Sets may mix both types.  Any other bit: OP_ERR_INVALID, before any device work.
	 * Accepted by op_blend, op_blend_gains, op_blend_block_gains, op_blend_vignette and the three overlap passes. */
	int on_device;
	double homo_inv[9];   /* ImageComponent::homo_inv (stitch/stitcher_image.hh:40-42) */
	double range[4];      /* ImageComponent::range: min.x, min.y, max.x, max.y (:48) */
	/* Dimensions of the pixel buffer `data` when they differ from h / w, else 0.  The reference keeps
	 * ImageRef::_width/_height from load() (stitch/imageref.hh:22-31) after CylinderStitcher replaced the
	 * Mat by its cylinder warp (cylstitcher.cc:66-67): bounds, blend weights and the image centre keep
	 * using the ORIGINAL size (blender.hh:39-44, blender.cc:31-35, stitcher_image.cc:150) while
	 * interpolate() reads the warped Mat with its own rows/cols (lib/imgproc.cc:135-156).  h / w are the
	 * ImageRef's, mat_h / mat_w the Mat's. */
	int mat_h, mat_w;
} op_blend_image;
typedef struct op_blend_geom {
	int proj_method;      /* ConnectedImages::ProjectionMethod (:30): 0 flat, 1 cylindrical, 2 spherical */
	double proj_min[2], proj_max[2];   /* ConnectedImages::proj_range (:33) */
	double resolution[2];              /* ConnectedImages::get_final_resolution() (stitcher_image.cc:79-114) */
} op_blend_geom;
/* HOST-side O(n) geometry the reference also runs on the host, in fp64 with the host libm:
 * calc_inverse_homo + update_proj_range + get_final_resolution (stitcher_image.cc:36-114).
 * homo: n x 9 ImageComponent::homo; shapes_wh: n x (w, h).  Fills g, homo_inv (n x 9) and
 * ranges (n x 4).  OP_ERR_INVALID where the reference would m_assert / error_exit. */
int op_blend_prepare(const op_config* cfg, int proj_method, int identity_idx, int n, const int* shapes_wh,
		const double* homo, op_blend_geom* g, double* homo_inv, double* ranges);
/* canvas size LinearBlender/MultiBandBlender::add_image arrive at (blender.cc:15-22) */
int op_blend_canvas_dims(const op_blend_geom* g, const op_blend_image* imgs, int n, int* h, int* w);
typedef struct op_canvas op_canvas;   /* device-resident H x W x 3 fp32 result (Mat32f) */
int op_blend(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, op_canvas** out);
int op_canvas_dims(const op_canvas* c, int* h, int* w);
const float* op_canvas_device(const op_canvas* c);
int op_canvas_copy(op_ctx* ctx, const op_canvas* c, float* host);
void op_canvas_free(op_canvas* c);
/* crop(mat) (lib/imgproc.cc:200-235, called by main.cc:226-229 under config CROP): the largest
 * rectangle of valid pixels, first maximum in (line, column) scan order like the reference.
 * x0 / y0 (optional) receive the rectangle's origin in c.  The result may be empty (h = 0). */
int op_canvas_crop(op_ctx* ctx, const op_canvas* c, op_canvas** out, int* x0, int* y0);
/* write_rgb / write_png quantisation (lib/imgio.cc:25-40,98-113): Color::NO -> white, v * 255
 * truncated to a byte; D2H of H x W x 3 bytes instead of the fp32 canvas */
int op_canvas_copy_u8(op_ctx* ctx, const op_canvas* c, unsigned char* host);

/* ---- EXPOSURE (GAIN) COMPENSATION -- an extension beyond the reference, which asks for fixed exposure instead (README,
 * Quality Guidelines): the gain compensation of Brown & Lowe, "Automatic Panoramic Image Stitching using Invariant
 * Features" (IJCV 2007, section 6).  Opt-in: op_blend itself is unchanged.
 *
 * Pairs (a < b) of n images are stored at index  a*n - a*(a+1)/2 + (b - a - 1),  n*(n-1)/2 entries.
 *
 * op_gain_overlap: overlap statistics over the canvas op_blend would produce, on the lattice of canvas pixels whose row and
 * column are multiples of `stride` (>= 1).  At each such pixel every image whose sample is valid by the LINEAR blender's
 * rules (cfg->LAZY_READ's ROI test, map_coor bounds, interpolate() != NO, col[0] >= 0 -- whatever cfg->MULTIBAND says)
 * takes part; for every pair (a < b) of them: count[p] += 1, sums[6p + c] += col_a[c], sums[6p + 3 + c] += col_b[c]
 * (c = 0..2), colours in fixed point llrint(col * 2^32) summed in int64: the result does not depend on the order of the
 * device's additions (bit-equal between runs).  Images are expected in [0, 1].  count / sums may be NULL when n == 1.
 * At most 262144 images (OP_ERR_UNSUPPORTED beyond).
 * op_gain_solve (HOST ONLY, no device): the gains minimising
 *   e = 1/2 sum_a sum_{b!=a} N_ab [ (g_a I_ab - g_b I_ba)^2 / sigma_n^2 + (1 - g_a)^2 / sigma_g^2 ],  I_ab = S_ab / (2^32 N_ab),
 * intensities in [0, 1] units (usual sigma_n = 10/255, sigma_g = 0.1).  per_channel = 1: one solve per channel;
 * 0: one solve on the grey mean (S[0]+S[1]+S[2]) / 3, the same gain for all three channels.  An image without overlap
 * gets 1.  gains: n x 3.
 * op_blend_gains: op_blend with every valid sample scaled, col[c] = min(col[c] * gains[3k + c], 1) -- in the linear
 * blender and in the multiband blender's level 0 -- where a channel whose gain is exactly 1 is left as it is.  gains:
 * n x 3 host floats, finite and > 0; NULL = op_blend.  All-ones gains give op_blend's canvas bit for bit.
 * Bad arguments (NULLs, n < 1, stride < 1, non-positive or non-finite sigmas / gains) return OP_ERR_INVALID.
 * Threading and ownership as op_blend: one call at a time per context; the caller owns count / sums / gains and the
 * returned canvas (op_canvas_free). */
int op_gain_overlap(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int stride,
		int64_t* count, int64_t* sums);
int op_gain_solve(int n, const int64_t* count, const int64_t* sums, double sigma_n, double sigma_g, int per_channel, float* gains);
int op_blend_gains(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n,
		const float* gains, op_canvas** out);

/* ---- BLOCK GAIN COMPENSATION (ABI 10) -- the gains above, one per block of a bx x by grid on every image instead of one
 * per image (as OpenCV's BlocksGainCompensator): it also evens out brightness that varies INSIDE a view (vignetting, sky
 * gradients, metering).  Opt-in; bx = by = 1 reduces exactly to the per-image entry points.
 *
 * Blocks.  Image k (op_blend_image h x w -- the ImageRef size, also after a cylinder pre-warp) is split into bx x by blocks,
 * bx, by in [1, 16], B = bx * by; unit (k, q), q = v * bx + u, is block (u, v) of image k.  A sample at image coordinates
 * (r, c) -- the floats the linear blender passes to interpolate() -- lies in block, in fp32 exactly,
 *   u = clamp((int)floorf(c * (float)bx / (float)w), 0, bx - 1),   v = clamp((int)floorf(r * (float)by / (float)h), 0, by - 1).
 *
 * op_gain_block_overlap: op_gain_overlap's statistics (same lattice, validity rules, LAZY_READ branches, fixed point)
 * split by block pair: pair p (a < b, index as above) and blocks (qa, qb) of its samples at entry e = p * B^2 + qa * B + qb:
 * count[e], sums[6e .. 6e + 5] = S_ab[3], S_ba[3].  count: P * B^2, sums: P * B^2 * 6 (P = n (n - 1) / 2; both may be NULL
 * when n == 1).  At most 2^22 entries P * B^2 (OP_ERR_UNSUPPORTED beyond; 128 images at 4 x 4 use 2.1 M).
 * op_gain_block_solve (HOST ONLY): the unit gains minimising
 *   e = 1/2 sum_{unit pairs (a,qa),(b,qb), a != b} N [ (g_{a,qa} I - g_{b,qb} I')^2 / sigma_n^2 + (1 - g_{a,qa})^2 / sigma_g^2 ]
 *     + 1/2 sum_k sum_{4-neighbour blocks q ~ q'} lambda_k (g_{k,q} - g_{k,q'})^2 / sigma_s^2,     lambda_k = M_k / B,
 * both sums over ordered pairs (every edge counts twice, like every unit pair), N / I / I' the count and means of the
 * entry, M_k the overlap count of image k over all its pairs (the smoothness term in the data term's sample units).
 * Every unit of an image with any overlap is unknown -- a block that overlaps nothing takes its gain from its neighbours
 * through the smoothness term; an image without overlap gets 1.  Usual sigma_s = 0.1.  per_channel as op_gain_solve.
 * gains: n * by * bx * 3, gains[((k * by + v) * bx + u) * 3 + c].  fp64 dense Cholesky, fixed order; with bx = by = 1 the
 * floats of op_gain_solve.  At most n * B = 4096 units (OP_ERR_UNSUPPORTED beyond).
 * op_blend_block_gains: op_blend with every valid sample (linear blender; multiband level 0) of image k at (r, c) scaled
 * by its block-centre gains interpolated bilinearly in fp32, clamped at the border:
 *   fx = c * (float)bx / (float)w - 0.5f, u0 = clamp(floorf(fx), 0, bx - 1), u1 = min(u0 + 1, bx - 1),
 *   tx = clamp(fx - u0, 0, 1) (the same for y), lerp(a, b, t) = a + t * (b - a),
 *   g = lerp(lerp(G[v0][u0], G[v0][u1], tx), lerp(G[v1][u0], G[v1][u1], tx), ty),
 * then col[c] = min(col[c] * g, 1), a channel whose g is exactly 1 left as it is.  A uniform map G_k gives
 * op_blend_gains(G)'s canvas bit for bit; NULL = op_blend.  gains finite and > 0.
 * Bad arguments (NULLs, n < 1, stride < 1, bx / by outside [1, 16], non-positive or non-finite sigmas / gains) return
 * OP_ERR_INVALID.  Threading and ownership as the per-image entry points. */
int op_gain_block_overlap(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int stride,
		int bx, int by, int64_t* count, int64_t* sums);
int op_gain_block_solve(int n, int bx, int by, const int64_t* count, const int64_t* sums, double sigma_n, double sigma_g, double sigma_s,
		int per_channel, float* gains);
int op_blend_block_gains(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int bx, int by,
		const float* gains, op_canvas** out);

/* ---- VIGNETTING COMPENSATION (ABI 11) -- exposure gains plus ONE radial falloff curve shared by all views (one lens, one
 * zoom and aperture setting), as Goldman (PAMI 2010) and Hugin's photometric optimiser add after Brown & Lowe's gains: a
 * scene point seen near the edge of one view and near the centre of another constrains the curve, so a panorama-wide
 * falloff that block gains cannot see is corrected.  Opt-in; a = 0 reduces exactly to op_blend_gains.
 *
 * Model.  Image k (op_blend_image h x w, the ImageRef size linear_sample bounds against) has its centre where the map puts
 * it, (0.5 w, 0.5 h).  A sample at image coordinates (r, c) -- the floats the linear blender passes to interpolate() -- has
 * the normalised squared radius, in fp32 exactly (fw = (float)w, fh = (float)h),
 *   dx = c - 0.5f * fw,  dy = r - 0.5f * fh,  rho = fminf((dx * dx + dy * dy) / (0.25f * (fw * fw + fh * fh)), 1.f),
 * in [0, 1], isotropic in pixels, 1 at the corners; and the grey level Y = (col[0] + col[1] + col[2]) / 3.f.  Observation
 * model: Y_k(x) = e_k V(rho_k(x)) L(x), V(rho) = 1 + a1 rho + a2 rho^2 + a3 rho^3, achromatic; gains g_k = 1 / e_k are grey.
 * Views whose mat_h / mat_w are set to another size than h / w (a cylinder pre-warp) are refused with OP_ERR_UNSUPPORTED:
 * their samples are not in the lens frame.
 *
 * op_vignette_overlap: op_gain_overlap's lattice, validity rules and LAZY_READ branches; a sample whose largest channel
 * exceeds clip (in (0, 1]; 1 keeps every valid sample of an image in [0, 1]) does not take part.  For every pair p (a < b,
 * index as above) of valid samples, pa[k] = rho_a^k and pb[k] = rho_b^k in fp64 (pa[0] = 1, pa[k] = pa[k-1] * rho_a):
 *   count[p] += 1,
 *   moments[30p + k]          = A_k  += (Ya * Ya) * pb[k]            k = 0..6
 *   moments[30p + 7 + k]      = B_k  += (Yb * Yb) * pa[k]            k = 0..6
 *   moments[30p + 14 + 4i + j] = C_ij += ((Ya * Yb) * pa[i]) * pb[j]  i, j = 0..3
 * each product formed in fp64 from the fp32 Y / rho in that order and summed as llrint(x * 2^32) in int64 (bit-equal
 * between runs).  Every term lies in [0, 1]; at most 2^30 lattice points per call (OP_ERR_UNSUPPORTED beyond: raise the
 * stride), so no sum can overflow.  count: P, moments: 30 P (both may be NULL when n == 1).
 * op_vignette_solve (HOST ONLY): gains and the curve minimising, a = (1, a1, a2, a3), H(A) the 4 x 4 Hankel matrix A_{i+j},
 *   E = sum_p [ (g_a^2 a'H(A)a - 2 g_a g_b a'Ca + g_b^2 a'H(B)a) / sigma_n^2 + N_p ((1 - g_a)^2 + (1 - g_b)^2) / sigma_g^2 ]
 *     + (sum_p N_p) (a1^2 + a2^2 + a3^2) / sigma_v^2,
 * the data term being sum (g_a Y_a V(rho_b) - g_b Y_b V(rho_a))^2 over the pair's samples (moments in 2^-32 units).
 * Alternation from a = 0: g given a (an SPD system with op_gain_solve's pattern), then a1..a_degree given g (the others stay
 * 0); at most 100 rounds, stopping early when a round lowers E by no more than 1e-12 E.  The gains are then divided by
 * their overlap-weighted mean sum_p N_p (g_a + g_b) / (2 sum_p N_p): the data term pulls all of them towards 0 where the
 * overlaps disagree with the model, and this keeps the panorama's brightness (ratios and curve unchanged).  fp64, fixed
 * order.  degree in [1, 3].  Usual sigma_n = 10/255, sigma_g = 1, sigma_v = 100 (the weak priors a one-row sweep needs).
 * gains: n x 3, the same gain in all three channels; images without overlap get 1; no overlap at all: a = 0.
 * poly: a1, a2, a3.  OP_ERR_UNSUPPORTED (gains 1, poly 0 written) when the fitted curve does not stay above 1e-6 on
 * [0, 1] or a gain is not positive: the caller keeps plain gains.
 * op_blend_vignette: op_blend with every valid sample (linear blender; multiband level 0) of image k at (r, c) scaled by
 *   V = 1.f + rho * (a1 + rho * (a2 + rho * a3)),  f_c = gains[3k + c] / V  (fp32),  col[c] = min(col[c] * f_c, 1),
 * a channel whose f_c is exactly 1 left as it is.  gains NULL = all 1, poly NULL = 0; gains finite and > 0, the curve above
 * 1e-6 on [0, 1].  a = 0 gives op_blend_gains(gains)'s canvas bit for bit, and with gains 1 op_blend's.
 * Bad arguments return OP_ERR_INVALID.  Threading and ownership as the per-image entry points. */
int op_vignette_overlap(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, int stride,
		float clip, int64_t* count, int64_t* moments);
int op_vignette_solve(int n, const int64_t* count, const int64_t* moments, int degree, double sigma_n, double sigma_g, double sigma_v,
		float* gains, float* poly);
int op_blend_vignette(op_ctx* ctx, const op_config* cfg, const op_blend_geom* g, const op_blend_image* imgs, int n, const float* gains,
		const float* poly, op_canvas** out);

/* ---- PNG OUTPUT (ABI 12) -- replaces write_rgb(fname, mat) and the encoder behind it, write_png -> lodepng::encode
 * (lib/imgio.cc:25-41,98-113; called by main.cc:226-233), the largest single cost of a whole run of the reference's CLI.
 * The canvas is quantised, filtered, deflated and framed on the device; one D2H brings back the finished file.
 * Format: 8-bit RGB (colour type 2), no interlace, no ancillary chunks: signature, IHDR, IDAT chunks, IEND.  The pixels are
 * op_canvas_copy_u8's bytes (Color::NO -> 255, v * 255 truncated); the reference hands lodepng RGBA with alpha 255, which
 * lodepng's colour reduction stores as RGB, so a decoder sees the same pixels from both files.  The IDAT payload is one zlib
 * stream; the file is a function of the pixels alone (bit-equal between runs, contexts and devices): DESIGN.md section 11
 * gives the parse and the Huffman construction, tests/harness/png_ref.c restates them serially.
 * op_canvas_encode_png: the device-resident canvas of op_blend / op_canvas_crop.  An empty canvas (h = 0 or w = 0, which
 * op_canvas_crop can return) is OP_ERR_INVALID: the format has no zero-sized image.  (lib/imgio.cc:25-41,98-113)
 * op_png_encode_u8: the same encoder for H x W x 3 bytes in host memory -- what the reference's main.cc holds after
 * write_rgb's quantisation loop (lib/imgio.cc:25-41,98-113).
 * op_png_size / op_png_copy: the file's length and its bytes (host must have room for op_png_size bytes; lib/imgio.cc:98-113
 * hands them to lodepng's file writer).  op_png_free releases the object.  Filtered streams above 4 GiB: OP_ERR_UNSUPPORTED.
 * Threading and ownership as op_blend: one call at a time per context; the caller owns the returned op_png. */
typedef struct op_png op_png;
int op_canvas_encode_png(op_ctx* ctx, const op_canvas* c, op_png** out);
int op_png_encode_u8(op_ctx* ctx, const unsigned char* rgb_host, int h, int w, op_png** out);
int64_t op_png_size(const op_png* p);
int op_png_copy(op_ctx* ctx, const op_png* p, unsigned char* host);
void op_png_free(op_png* p);

/* ---- JPEG OUTPUT (additive within ABI 12) -- replaces write_rgb(fname, mat) where the build writes out.jpg: CImg's save_jpeg
 * and libjpeg behind it (lib/imgio.cc:98-113; called by main.cc:30,233).  The canvas is quantised, colour-converted,
 * transformed, Huffman-coded and byte-stuffed on the device; one D2H brings back the entropy-coded data.
 * Format: baseline sequential DCT, 8 bits, JFIF 1.1, YCbCr at 4:4:4 or 4:2:0, the quantisation tables libjpeg derives from
 * `quality` (the reference's file is quality 100, 4:2:0), the Huffman tables of ITU T.81 Annex K.3, a restart marker every
 * 32 (4:4:4) or 8 (4:2:0) MCUs.  Every byte is what libjpeg writes for the same pixels, quality, sampling and restart
 * interval; the pixels are op_canvas_copy_u8's bytes (Color::NO -> 255, v * 255 truncated).  The file is a function of the
 * pixels alone: DESIGN.md section 13 gives the rules, tests/harness/jpeg_ref.c restates them serially.
 * op_canvas_encode_jpeg: the device-resident canvas of op_blend / op_canvas_crop (lib/imgio.cc:98-113, main.cc:226-233).
 * quality outside 1..100, an unknown subsampling or an empty canvas (h = 0 or w = 0, which op_canvas_crop can return) is
 * OP_ERR_INVALID; h or w above 65535 (the frame header's 16-bit fields) is OP_ERR_UNSUPPORTED, before anything is allocated.
 * op_jpeg_encode_u8: the same encoder for H x W x 3 bytes in host memory -- what write_rgb holds after its quantisation
 * loop (lib/imgio.cc:98-113).
 * op_jpeg_size / op_jpeg_copy: the file's length and its bytes (host must have room for op_jpeg_size bytes; lib/imgio.cc:98-113
 * hands them to libjpeg's stdio destination).  op_jpeg_free releases the object.
 * Threading and ownership as op_png: one call at a time per context; the caller owns the returned op_jpeg. */
typedef struct op_jpeg op_jpeg;
enum { OP_JPEG_444 = 0, OP_JPEG_420 = 1, OP_JPEG_422 = 2, OP_JPEG_GREY = 3 };      /* the encoder takes the first two; op_jpeg_probe reports all four */
int op_canvas_encode_jpeg(op_ctx* ctx, const op_canvas* c, int quality, int subsampling, op_jpeg** out);
int op_jpeg_encode_u8(op_ctx* ctx, const unsigned char* rgb_host, int h, int w, int quality, int subsampling, op_jpeg** out);
int64_t op_jpeg_size(const op_jpeg* p);
int op_jpeg_copy(op_ctx* ctx, const op_jpeg* p, unsigned char* host);
void op_jpeg_free(op_jpeg* p);

/* CYLINDER mode pre-warp -- replaces CylinderWarper::warp (stitch/warp.hh:47-55, warp.cc:13-75).
 * op_cyl_warp_shape is the host part (projector, output shape, offset and the keypoints, which
 * are centred coordinates updated in place: warp.cc:46-67); op_cyl_warp renders the pixels.  The image may be OP_F32 or
 * OP_U8 (bytes converted in the sampler as for OP_SRC_U8); the result is the same fp32 canvas either way. */
int op_cyl_warp_shape(const op_config* cfg, int w, int h, double h_factor, double* pts, int npts,
		int* new_w, int* new_h, double* offset);
int op_cyl_warp(op_ctx* ctx, const op_config* cfg, const op_image* img, double h_factor, op_canvas** out);

/* CYLINDER mode perspective correction (additive within ABI 12) -- replaces CylinderStitcher::perspective_correction
 * (stitch/cylstitcher.cc:139-180), the last pixel stage of CylinderStitcher::build(): the blended canvas never leaves the device.
 * op_canvas_upload: a device canvas from an h x w x 3 fp32 host image (a Mat32f; Color::NO = -1 allowed).  NULLs, h < 1 or
 * w < 1 return OP_ERR_INVALID before any device work.
 * op_perspective_homography (host only, fp64): the geometry of :140-168.  The corners (-0.5, -0.5), (-0.5, 0.5) of the bundle's
 * first component and (0.5, -0.5), (0.5, 0.5) of its last go through to_ref_coor -- times the component's ImageRef size (the
 * stale one after the pre-warp, not the Mat's), homo.trans, x / ref_w and y / ref_h, the flat homo2proj, times ref_w / ref_h,
 * minus g->proj_min -- and inv is the homography that maps (0, 0), (0, canvas_h), (canvas_w, 0), (canvas_w, canvas_h) onto them
 * in that order, h33 = 1: getPerspectiveTransform(corners, corners_std), solved by the routine RANSAC's 4-point model uses
 * (the reference: Eigen's JacobiSVD, so its inv differs in the last digits).  corners (optional) receives the four corners as
 * x, y pairs.  NULLs, a size below 1, three corners on one line or a non-finite entry in inv return OP_ERR_INVALID.
 * op_canvas_perspective: the LinearBlender pass of :170-179 over the canvas itself -- one image, ROI (0, 0)-(w, h), output of
 * the same size.  Output pixel (i, j) samples c at Homography::trans2d(j, i) (no centre offset, no z < 0 test; map_coor's
 * bounds on the doubles), weighted as LinearBlender::run does under cfg->ORDERED_INPUT and divided as its cfg->LAZY_READ branch
 * does: the reference's pixels, bit for bit, for the same inv.  A non-finite entry in inv returns OP_ERR_INVALID before any
 * device work; an empty canvas gives an empty canvas. */
int op_canvas_upload(op_ctx* ctx, const float* host_rgb, int h, int w, op_canvas** out);
int op_perspective_homography(const op_blend_geom* g, int ref_w, int ref_h, int first_w, int first_h, const double* first_homo,
		int last_w, int last_h, const double* last_homo, int canvas_w, int canvas_h, double* inv, double* corners);
int op_canvas_perspective(op_ctx* ctx, const op_config* cfg, const op_canvas* c, const double* inv, op_canvas** out);

/* ---- RESIDENT VIEWS -- the seam of ImageRef::load / ImageRef::img (stitch/imageref.hh:15-31): the reference loads every
 * view once and every stage reads that Mat.  An op_views holds the views of a job in library-owned device memory, each in
 * the type it arrived in (OP_F32 or OP_U8), so that SIFT, the cylinder warp, the overlap passes and every blend read ONE
 * upload: decoder bytes are a quarter of the PCIe and HBM traffic of their fp32 form and give the same results bit for bit.
 * op_views_upload: copies n host or device images (op_image; on_device 0 or 1); host images of one size at one constant
 * stride go up in one copy, as in op_sift_batch.  The sources are free again when it returns.
 * op_views_image: view i as a device op_image, for op_sift_batch / op_cyl_warp.
 * op_views_blend_image: fills data, h, w, the flag word and mat_h = mat_w = 0 of *out; homo_inv and range are left alone.
 * op_views_count: the number of views.  Bad arguments (NULLs, n < 1, an index out of range, sizes below 2, an unknown
 * dtype) return OP_ERR_INVALID, before any device work.
 * op_views_free: waits for the stream of the context the views were uploaded with, then releases the memory; every
 * op_image / op_blend_image taken from the object dangles afterwards.  An op_views must not outlive its context.
 * Threading as the rest: one call at a time per context. */
typedef struct op_views op_views;
int op_views_upload(op_ctx* ctx, const op_image* imgs, int n, op_views** out);
int op_views_count(const op_views* v);
int op_views_image(const op_views* v, int i, op_image* out);
int op_views_blend_image(const op_views* v, int i, op_blend_image* out);
void op_views_free(op_views* v);

/* ---- JPEG INPUT (additive within ABI 12) -- replaces read_img(fname) and the decoder behind it, CImg::load -> libjpeg
 * (lib/imgio.cc:67-90), where ImageRef::load calls it (stitch/imageref.hh:22-27): camera files go in, resident views come
 * out, and the decoded bytes never exist on the host.  DESIGN.md section 14 gives the format, the rules and the kernels;
 * tests/harness/jpeg_dec_ref.c restates the decoder serially.
 * Accepted: SOF0 (baseline sequential, Huffman, 8 bits) with one interleaved scan; three components as YCbCr at 4:4:4,
 * 4:2:2 (21 11 11) or 4:2:0 (22 11 11), or one component (grey, written R = G = B); any 8-bit DQT and any DHT tables; DRI
 * present or absent; APPn / COM segments of any content; bytes after EOI.  Every byte of a view is libjpeg's default decode of
 * the file (ISLOW IDCT, fancy upsampling, JFIF YCbCr -> RGB), i.e. the bytes lib/imgio.cc:78-80 converts to float.
 * OP_ERR_UNSUPPORTED: every other SOF, 12-bit precision, 16-bit DQT, other samplings or component counts, RGB components
 * (an Adobe APP14 with transform 0), more than one SOS, DNL.  OP_ERR_INVALID: a structurally broken header (a segment past
 * the end of the file, a missing SOF / DQT / DHT / SOS / EOI, a table id out of range), h or w below 2.  Both come from a
 * host parser that reads headers only, before anything is allocated or launched.
 * op_jpeg_probe (HOST ONLY, needs no device): parses `size` bytes at `file` and writes h, w and the sampling (OP_JPEG_444,
 * OP_JPEG_420, OP_JPEG_422 or OP_JPEG_GREY; each may be NULL).  OP_OK, OP_ERR_UNSUPPORTED or OP_ERR_INVALID, so a caller
 * can route a file to a decoder of its own (lib/imgio.cc:67-90).
 * op_views_decode_jpeg: decodes n files into one op_views of OP_U8 views, indistinguishable from op_views_upload of the
 * same bytes (stitch/imageref.hh:22-27).  All or nothing: a refused file, or one whose entropy-coded data is corrupt
 * (OP_ERR_INVALID, found on the device), leaves *out NULL and no device memory held; op_last_error names the file's index
 * in the batch and the reason.  The sources are free again on return.
 * op_views_copy: view i to host memory in its own type, 3 h w bytes or floats (the read-back of ImageRef::img,
 * stitch/imageref.hh:15-31; for tests and callers that keep a host copy).
 * op_debug_set_jpeg_subseq_bits: test hook like op_debug_set_desc_list_cap: the bits of a subsequence of the parallel
 * Huffman decode, a multiple of 32 from 32 to 65536, or 0 for the default (1024).  The views do not depend on it.
 * op_debug_jpeg_last_rounds: test hook: the synchronisation rounds the last op_views_decode_jpeg on ctx needed (the
 * largest of its files).
 * Threading and ownership as op_views_upload: one call at a time per context; the caller frees the op_views. */
int op_jpeg_probe(const unsigned char* file, int64_t size, int* h, int* w, int* sampling);
int op_views_decode_jpeg(op_ctx* ctx, const unsigned char* const* files, const int64_t* sizes, int n, op_views** out);
int op_views_copy(op_ctx* ctx, const op_views* v, int i, void* host);
int op_debug_set_jpeg_subseq_bits(op_ctx* ctx, int bits);
int op_debug_jpeg_last_rounds(op_ctx* ctx);

/* ---- EXIF ORIENTATION (additive within ABI 12) -- an opt-in beyond the reference, whose decoder (CImg -> libjpeg,
 * lib/imgio.cc:67-90) ignores the tag: cameras store a portrait shot as a landscape frame and record the turn in EXIF tag
 * 0x0112, so op_views_decode_jpeg yields such a view lying on its side.  DESIGN.md section 17 gives the reader's rules and
 * the kernel.
 * op_jpeg_exif (HOST ONLY, needs no device): orientation 1..8 (1 when absent or unreadable) and FocalLengthIn35mmFilm in mm
 * (tag 0xA405; 0 when absent or unknown) -- the value the reference has users type into config.cfg as FOCAL_LENGTH
 * (config.cfg:14, read by stitch/warp.cc:72).  Either pointer may be NULL.  The reader walks the segments from SOI to the first SOS, takes the first
 * APP1 that starts with "Exif\0\0" and holds 8 more bytes, and visits IFD0 and the Exif sub-IFD (tag 0x8769) only, every
 * offset checked against the end of that segment.  Malformed EXIF is never an error: it gives 1, 0 and OP_OK.
 * OP_ERR_INVALID only for a NULL file, a negative size, or a file without SOI (as op_jpeg_probe).
 * op_views_decode_jpeg_oriented: op_views_decode_jpeg with every view turned upright.  orientation == NULL: every file's own
 * EXIF orientation.  Otherwise orientation[i] in 1..8 is used as given and 0 means "this file's EXIF"; any other value is
 * OP_ERR_INVALID before anything is allocated.  With s the stored h x w frame (op_views_decode_jpeg's view) and o view i:
 *   1: o[y][x] = s[y][x]            2: s[y][w-1-x]        3: s[h-1-y][w-1-x]      4: s[h-1-y][x]         (h x w)
 *   5: o[y][x] = s[x][y]            6: s[h-1-x][y]        7: s[h-1-x][w-1-y]      8: s[x][w-1-y]         (w x h)
 * which is what viewers do with the tag.  View i is OP_U8; op_views_image and op_views_copy report the turned shape.
 * Everything else as op_views_decode_jpeg: all or nothing, op_last_error names the failing index, a failed call holds no
 * device memory.  A call whose resolved orientations are all 1 runs op_views_decode_jpeg's launches and nothing else. */
int op_jpeg_exif(const unsigned char* file, int64_t size, int* orientation, int* focal35);
int op_views_decode_jpeg_oriented(op_ctx* ctx, const unsigned char* const* files, const int64_t* sizes, int n,
                                  const int* orientation, op_views** out);

/* ---- RE-PROJECTION OF A FINISHED PANORAMA (additive within ABI 12) -- replaces planet(fname) (main.cc:294-331), the one
 * thing the reference's CLI does with a finished panorama, and adds what it has no way to make: a rectilinear view in a chosen
 * direction and the six faces of a cube.  Each is a pure gather from an equirectangular canvas, one thread per output pixel;
 * the canvas stays on the device and the result is a canvas like any other (crop, PNG and JPEG output take it).  DESIGN.md
 * section 19 gives the maps; tests/reproject_cases.py restates them in numpy, and the device equals that restatement bit for
 * bit: the per-pixel angle is pano_atan2 (csrc/pano_angle.hpp: + - * / only, within 4e-15 rad of atan2), the square root is
 * correctly rounded on both sides, the colour arithmetic is interpolate's fp32 sequence (lib/imgproc.cc:135-156).
 *
 * op_pano_frame: where the canvas sits on the sphere.  Column c is longitude lon0 + c * step_lon, row r is latitude
 * lat0 + r * step_lat, y down as spherical::homo2proj gives them (projection.hh:50-52).  wrap = 1 is the caller's statement
 * that the W columns span exactly one turn (what planet assumes): step_lon is then ignored, a longitude d past lon0, brought
 * into [0, 2 pi), lies at column d / (M_PI * 2) * W, and the taps right of the last column read column 0.  lon0 must then
 * lie in [-pi, pi].  wrap is never guessed by the library.
 * op_view_spec: what to make.  OP_VIEW_PLANET: the reference's loop operation by operation on an out_h = out_w = OUTSIZE
 * square (main.cc:297-329; with wrap = 0 including its one-column seam of Color::NO where theta reaches w - 1); rot and focal
 * are not read, and of the frame only wrap.  OP_VIEW_RECTILINEAR: a pinhole camera.  Output pixel (i, j) looks along
 * d = rot * (j - (out_w - 1) / 2, i - (out_h - 1) / 2, focal), rot row-major, in the canvas's frame: x right, y down,
 * z forward (longitude 0, latitude 0); lon = atan2(d.x, d.z), lat = atan2(d.y, hypot(d.x, d.z)).  A pixel that looks outside
 * the canvas, or whose four taps touch Color::NO, is Color::NO.
 * op_pano_frame_of (HOST ONLY): the frame of the canvas a spherical blend made from geometry g, or of its crop at
 * (x0, y0): lon0 = proj_min[0] + x0 * resolution[0], lat0 likewise, the steps are the resolutions, wrap = 0.  Other
 * projections: OP_ERR_UNSUPPORTED.
 * op_view_look (HOST ONLY, host libm): rot = R_yaw (about y) * R_pitch (about x) * R_roll (about z), angles in radians, with
 *   R_yaw = [c 0 s; 0 1 0; -s 0 c],  R_pitch = [1 0 0; 0 c -s; 0 s c],  R_roll = [c -s 0; s c 0; 0 0 1]:
 * the optical axis is (sin yaw cos pitch, -sin pitch, cos yaw cos pitch), so positive yaw looks right and positive pitch looks
 * up (towards -y).  focal = 0.5 * out_w / tan(0.5 * hfov).  Non-finite angles, hfov outside (0, pi) and sizes below 1:
 * OP_ERR_INVALID.
 * op_view_cube_face (HOST ONLY): face 0..5 = +x, -x, +y, -y, +z, -z as an n x n rectilinear view with focal = 0.5 * n and a
 * signed permutation matrix (entries exactly 0, 1, -1).  The side faces +x, -x, +z, -z have -y (the zenith) at the top of the
 * picture; +y (looking down) has +z at the top, -y (looking up) has -z at the top: the faces of an unfolded cross around +z.
 * op_view_planet (HOST ONLY): the planet of n x n pixels (rot = identity, focal = 1, neither read).
 * op_canvas_reproject: the view `s` of canvas `c` lying at `f`, as a new out_h x out_w canvas.  NULLs, an unknown mode, a size
 * below 1, a planet that is not square, a non-finite field of f or s, focal <= 0, step_lat = 0, step_lon = 0 without wrap,
 * a wrap other than 0 or 1, or wrap with lon0 outside [-pi, pi] return OP_ERR_INVALID before any device work, with nothing
 * allocated.  An empty source gives a canvas of Color::NO.  Threading and ownership as op_blend: one call at a time per context; the caller frees the canvas. */
typedef struct op_pano_frame { double lon0, lat0, step_lon, step_lat; int wrap; } op_pano_frame;
typedef struct op_view_spec { int mode, out_h, out_w; double rot[9], focal; } op_view_spec;
enum { OP_VIEW_PLANET = 0, OP_VIEW_RECTILINEAR = 1 };
int op_pano_frame_of(const op_blend_geom* g, int x0, int y0, op_pano_frame* f);
int op_view_look(double yaw, double pitch, double roll, double hfov, int out_w, int out_h, op_view_spec* s);
int op_view_cube_face(int face, int n, op_view_spec* s);
int op_view_planet(int n, op_view_spec* s);
int op_canvas_reproject(op_ctx* ctx, const op_canvas* c, const op_pano_frame* f, const op_view_spec* s, op_canvas** out);

#ifdef __cplusplus
}
#endif
#endif /* OPENPANO_HIP_H */
