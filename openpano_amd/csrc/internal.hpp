// internal.hpp -- shared host/device declarations of libopenpano_hip.so (not part of the ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>
#include "openpano_hip.h"
#include "op_base.hpp"       // op_set_error, OP_FAIL, OP_MAX_KCENTER: the host-only units see them without the HIP runtime
#include "sift_plan.hpp"     // OctDesc, SiftPlan, plane_off_*: shared with the host-only sift_plan.cc

#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	op_set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); return OP_ERR_HIP; } } while (0)

// grow-only device scratch (hipMalloc, not the pool): the arenas of a context and the SIFT workspace
struct DevScratch {
	void* p = nullptr; size_t cap = 0;
	hipError_t ensure(size_t bytes) {
		if (bytes <= cap) return hipSuccess;
		if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }   // hipFree waits for the device
		const size_t want = bytes + bytes / 8;
		hipError_t e = hipMalloc(&p, want);
		if (e != hipSuccess) return e;
		cap = want;
		return hipSuccess;
	}
	void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
};

// per-stage device timing (HIP events on the context's stream), the counterpart of the
// reference's TotalTimer table (lib/timer.hh:63-83); labels reuse the reference's where one exists
struct ProfStage { std::string label; double total_ms = 0; long calls = 0; };
struct op_ctx {
	int device = 0;
	int num_cu = 256;                                // compute units of the device (sizes the persistent launches)
	hipStream_t stream = nullptr;
	bool owns_stream = false;
	bool profiling = false;
	int jpeg_subseq_bits = 0;                        // JPEG decoder: bits of a subsequence (0: JD_S_DEFAULT; op_debug_set_jpeg_subseq_bits)
	int jpeg_last_rounds = 0;                        // pass-B rounds of the last op_views_decode_jpeg (the largest of its images)
	std::string prof_only;                           // when not empty: only this stage is bracketed by events
	int match_slow_seen[2] = {-1, -1};               // exact-scan rows (forward, reverse) of the previous op_match_pairs call: sizes the next launch
	std::vector<ProfStage> prof;
	std::vector<hipEvent_t> ev_pool;                 // recycled events
	struct Pending { int stage; hipEvent_t a, b; };
	std::vector<Pending> pending;                    // recorded, not yet resolved
	void* pinned = nullptr; size_t pinned_cap = 0;   // grow-only pinned host scratch for D2H results
	// grow-only device scratch of the matcher and of RANSAC: a call's temporaries live here, so kernels that are
	// still queued when the call returns (the per-pair sort into the result buffer) keep valid inputs -- the next
	// call on this context is ordered behind them on the same stream (contexts are thread-compatible)
	DevScratch match_arena, ransac_arena;
	// blend: the canvas -> space map's transcendentals, tabulated per canvas column / row by the HOST libm (blend.hip,
	// trig_tables): kept across calls with the same canvas geometry
	struct TrigTables {
		int method = -1, w1 = 0, h1 = 0; double minx = 0, miny = 0, resx = 0, resy = 0;
		DevScratch dev; std::vector<double> host;
	} blend_trig, cyl_trig;
	// copy streams of the host-image pipeline (op_sift_batch_host): uploads run ahead of the kernels, results leave behind them
	hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;
	// second compute stream of op_ransac_pairs (the pairs with few matches, whose sample tables take longest, run beside
	// the others) and the two events that fork it from / join it to the context's stream
	hipStream_t aux_stream = nullptr; hipEvent_t aux_fork = nullptr, aux_join = nullptr;
	hipError_t aux() {
		if (!aux_stream) { hipError_t e = hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking); if (e != hipSuccess) return e; }
		if (!aux_fork) { hipError_t e = hipEventCreateWithFlags(&aux_fork, hipEventDisableTiming); if (e != hipSuccess) return e; }
		if (!aux_join) { hipError_t e = hipEventCreateWithFlags(&aux_join, hipEventDisableTiming); if (e != hipSuccess) return e; }
		return hipSuccess;
	}
	hipError_t copy_streams() {
		if (!h2d_stream) { hipError_t e = hipStreamCreateWithFlags(&h2d_stream, hipStreamNonBlocking); if (e != hipSuccess) return e; }
		if (!d2h_stream) { hipError_t e = hipStreamCreateWithFlags(&d2h_stream, hipStreamNonBlocking); if (e != hipSuccess) return e; }
		return hipSuccess;
	}
	void* pinned_scratch(size_t bytes) {
		if (bytes <= pinned_cap) return pinned;
		if (pinned) hipHostFree(pinned);
		pinned = nullptr; pinned_cap = 0;
		if (hipHostMalloc(&pinned, bytes + bytes / 4) != hipSuccess) return nullptr;
		pinned_cap = bytes + bytes / 4;
		return pinned;
	}
	int prof_stage(const std::string& label) {
		for (size_t i = 0; i < prof.size(); ++i) if (prof[i].label == label) return (int)i;
		prof.push_back(ProfStage{label, 0, 0});
		return (int)prof.size() - 1;
	}
};
// RAII bracket around one stage's launches; resolve_profile() after a stream sync
struct ProfScope {
	op_ctx* c; int stage = -1; hipEvent_t a = nullptr, b = nullptr;
	ProfScope(op_ctx* ctx, const char* label);
	~ProfScope();
};
void resolve_profile(op_ctx* c);
// host-side wall time of a stage, reported in the same table (labels end in " (host)")
struct HostScope {
	op_ctx* c; const char* label; double t0;
	HostScope(op_ctx* ctx, const char* l);
	~HostScope();
};

// Host-side parallel loop over [0, n): a persistent pool of std::threads (the process may host
// several OpenMP runtimes -- PyTorch's, the reference's -- whose interplay cannot be relied on).
#include <functional>
// (`grain`: items a woken thread should find -- short items are not worth a thread each)
void host_parallel_for(int n, const std::function<void(int)>& body, int grain = 1);

// Size-class cache of device allocations (per device, process-wide, thread-safe): result buffers
// (op_features, op_canvas) and per-call temporaries come from here, so a steady-state call does
// no hipMalloc/hipFree (each costs tens of microseconds and synchronises the device).
hipError_t pool_alloc(void** p, size_t bytes);
void pool_free(void* p);
void pool_trim();     // release every cached block back to the runtime

// The pool does not track streams, so a block may go back to it only when the stream that last touched it is idle.
// CallBlocks is the one owner of the blocks (and events) a C-layer call allocates: made from the stream(s) the call works
// on, it frees what it still holds on every exit and waits for its streams first, unless the call's own last wait was
// finish() -- or settled() tells it of one.  A block that moves into a result handle is release()d on the call's last lines.
struct CallBlocks {
	std::vector<hipStream_t> streams; std::vector<void*> blocks; std::vector<hipEvent_t> events; bool idle = false;
	explicit CallBlocks(std::vector<hipStream_t> s): streams(std::move(s)) {}
	CallBlocks(const CallBlocks&) = delete; CallBlocks& operator=(const CallBlocks&) = delete;
	template <typename T> hipError_t alloc(T** p, size_t bytes) { hipError_t e = pool_alloc((void**)p, bytes); if (e == hipSuccess) blocks.push_back((void*)*p); return e; }
	hipError_t event() { hipEvent_t ev; hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming); if (e == hipSuccess) events.push_back(ev); return e; }      // events.back()
	// the caller (a result handle) owns p from here on
	template <typename T> T* release(T* p) { blocks.erase(std::remove(blocks.begin(), blocks.end(), (void*)p), blocks.end()); return p; }
	template <typename T> void free(T*& p) { pool_free(release(p)); p = nullptr; }      // at once: only behind a wait
	hipError_t finish() {                          // the call's last wait: hipStreamSynchronize of every stream, the first error returned
		hipError_t r = hipSuccess;
		for (hipStream_t s : streams) { hipError_t e = hipStreamSynchronize(s); if (r == hipSuccess) r = e; }
		idle = true;                               // a failed wait cannot be helped: the blocks are freed regardless
		return r;
	}
	void settled() { idle = true; }
	~CallBlocks() {
		if (!idle && !(blocks.empty() && events.empty())) (void)finish();
		for (void* b : blocks) pool_free(b);
		for (hipEvent_t e : events) hipEventDestroy(e);
	}
};
// waits for a forked stream when its scope ends between the fork (armed) and the join (disarmed)
struct StreamJoin { hipStream_t stream = nullptr; bool armed = false; ~StreamJoin() { if (armed) (void)hipStreamSynchronize(stream); } };

// the views of a job, resident on the device (op_views_upload in views.hip, op_views_decode_jpeg in jpeg_dec.hip)
struct op_views {
	op_ctx* ctx = nullptr;
	char* block = nullptr;            // one pool block; view i at imgs[i].data, a multiple of 256 bytes into it
	std::vector<op_image> imgs;       // device images, each in its own dtype
};

// a blended, warped or cropped image on the device (blend.hip and canvas.hip make them; canvas.hip, png.hip and jpeg.hip read them)
struct op_canvas {
	float* data = nullptr;   // device, h x w x 3
	int h = 0, w = 0;
	int device = 0;
};
// The byte of a canvas float: write_rgb / write_png quantisation (lib/imgio.cc:25-40,98-113), Color::NO -> white, float * 255
// truncated.  The one expression behind op_canvas_copy_u8 and the PNG and JPEG encoders, whose files are byte-equal to the
// reference's because of it.
__device__ __forceinline__ unsigned char canvas_byte(float v) { return (unsigned char)((v < 0 ? 1.f : v) * 255.f); }

// a scale-space point (feature/feature.hh:33-39), 48 bytes
struct KeyPoint {
	int x, y, oct, scale;
	double rx, ry;          // real_coor in [0,1)
	float dir, sf;          // dir, scale_factor
	int src;                // index of the raw candidate / refined parent
	int pad;
};

// ---- kernel launchers (each returns hipGetLastError of its launch) ----
// source -> grey base of every octave (working image only written when write_work: staged dump)
hipError_t launch_grey_octaves(const SiftPlan& p, bool write_work, hipStream_t st);
// fused scale space + extrema scan: fills the DoG / Gaussian planes and appends raw extrema
hipError_t launch_pyramid(const SiftPlan& p, int* raw /* n x cap x 4 */, int* raw_count /* n */, int cap, hipStream_t st);
size_t pyramid_lds_bytes(int halo);      // LDS of its generic kernel at a Gaussian half-width (run_group refuses a plan that does not fit)
// debug/staged dump only: mag and ort of one Gaussian plane (GaussianPyramid::cal_mag_ort)
hipError_t launch_magort_plane(const SiftPlan& p, int img, int oct, int s, float* mag, float* ort, hipStream_t st);
// expect = the largest per-image list length seen in the previous batch (0: unknown).  Workgroups cost dispatcher time
// whether they find work or not (k_refine over the whole 16 K capacity: 4864 workgroups for 30 busy ones per image took
// 35 us more than a grid sized to the lists), so k_refine, the ranking wavefronts of k_orientation and k_orient_peaks get as
// many workgroups as the expectation needs; all of them stride over their lists, any grid is correct.
hipError_t launch_refine(const SiftPlan& p, const int* raw, const int* raw_count, int cap, int expect,
		KeyPoint* refined /* n x cap */, int* refined_count, hipStream_t st);
// per_image[img * OP_OCNT_STRIDE] += orientation peaks of every keypoint (atomic; one counter per 128-byte line; cleared at the start of the step)
#define OP_OCNT_STRIDE 32
hipError_t launch_orientation(const SiftPlan& p, const KeyPoint* refined, const int* refined_count, int cap, int expect,
		float* dirs /* n x cap x 36: histogram in, peak directions out */, int* ndirs /* n x cap */, int* per_image /* n x OP_OCNT_STRIDE */,
		KeyPoint* sorted /* n x cap: refined in the canonical order */, int* slot_of /* n x cap: sorted position -> slot in refined */, hipStream_t st);
// image img's keypoints land at [sum of the earlier images' counts, ...); *total = sum of all, count_out[0..n) = the counts packed
// (device-side, no host round trip)
hipError_t launch_expand_oriented(const SiftPlan& p, const KeyPoint* sorted, const int* slot_of, const int* refined_count, int cap,
		const float* dirs, const int* ndirs, const int* per_image /* n x OP_OCNT_STRIDE */, long long* total, int* count_out /* n */,
		KeyPoint* oriented, long long oriented_cap, hipStream_t st);
// the descriptor count is read on the device (*total); cap = capacity of the output buffers
hipError_t launch_descriptor(const SiftPlan& p, const KeyPoint* oriented, const long long* total /* device */,
		long long cap, float* desc, double* coor, double* real, hipStream_t st);
hipError_t launch_debug_math(int which, const float* x, const float* y, int n, float* out, hipStream_t st);
