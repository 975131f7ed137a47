// features.hpp -- the feature table (op_features) and the three device arrays behind it, for the units that make tables:
// features.hip, sift_host.hip, sift_dump.hip.  Every other unit reads a table through handles.hpp.
#pragma once
#include "handles.hpp"
#include <mutex>

struct op_features {
	int n = 0;
	std::vector<int> counts;
	std::vector<int64_t> offsets;      // n + 1
	float* desc = nullptr;             // device, total x 128
	double* coor = nullptr;            // device, total x 2 (centred original-image pixels)
	double* real = nullptr;            // device, total x 2 (real_coor in [0,1)); null when built from host/device arrays
	bool has_desc = true;              // false: coordinates only (RANSAC-only use)
	bool owns = true;                  // false: desc / coor belong to the caller (op_features_adopt_device)
	int device = 0;
	// multi.hip: the same table on the other devices of an op_group (index = context of the group; [0] unused),
	// filled by the all-gather of op_sift_batch_multi / the first op_match_pairs_multi and owned by this object
	std::vector<op_features*> replicas;
	// host mirror of coor, fetched the first time a host stage asks for it (the acceptance epilogue of
	// op_ransac_pairs walks every keypoint of both images; features are immutable, so one copy serves every call)
	mutable std::vector<double> h_coor; mutable bool h_coor_valid = false; mutable std::mutex h_mu;
};

using FeaturesPtr = std::unique_ptr<op_features, void (*)(op_features*)>;       // a result handle is owned from birth
// n images, counts / offsets zeroed or (counts given) filled; null + error set on a negative count
FeaturesPtr new_features(int n, int device, const int* counts = nullptr);

// The three device arrays of a table, rows x (128 fp32 desc, 2 fp64 coor, 2 fp64 real): what run_group leaves and what every
// constructor of a table fills.  The blocks belong to the call's CallBlocks until dropped (a re-run) or handed to the op_features
// the call returns; of() is a view of arrays that a table owns already.
struct FeatArrays {
	std::vector<int> counts;          // run_group: per image of the group
	float* desc = nullptr; double* coor = nullptr; double* real = nullptr;   // device (pool), flat
	long long total = 0;
	static FeatArrays of(const float* desc, const double* coor, const double* real) {
		FeatArrays a; a.desc = const_cast<float*>(desc); a.coor = const_cast<double*>(coor); a.real = const_cast<double*>(real); return a;
	}
	static FeatArrays of(const op_features* f) { return of(f->has_desc ? f->desc : nullptr, f->coor, f->real); }
	hipError_t alloc(CallBlocks& own, size_t rows, bool with_desc = true, bool with_real = true) {
		hipError_t e = own.alloc(&desc, with_desc ? sizeof(float) * 128 * rows : sizeof(float));
		if (e == hipSuccess) e = own.alloc(&coor, sizeof(double) * 2 * rows);
		return e == hipSuccess && with_real ? own.alloc(&real, sizeof(double) * 2 * rows) : e;
	}
	// rows [src_row, src_row + rows) of src -> rows [dst_row, ..) of this, queued on st in the order desc, coor, real; an array that
	// either side lacks is left out.  Between devices (this on dst_dev, src on src_dev) the copies are peer copies.
	hipError_t copy_rows(int64_t dst_row, const FeatArrays& src, int64_t src_row, size_t rows, hipStream_t st, int dst_dev = 0, int src_dev = 0);
	void drop(CallBlocks& own) { own.free(desc); own.free(coor); own.free(real); }      // only behind a wait for the stream
	void hand_to(op_features* f, CallBlocks& own) { f->desc = own.release(desc); f->coor = own.release(coor); f->real = own.release(real); }
	int deliver(FeaturesPtr& f, CallBlocks& own, op_features** out) { HIPCHK(own.finish()); hand_to(f.get(), own); *out = f.release(); return OP_OK; }      // a call's last line
};
