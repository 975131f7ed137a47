// sift_host.hpp -- what sift_host.hip (the batched call) and sift_dump.hip (the staged dump) share: the workspace and run_group
#pragma once
#include "features.hpp"

struct Workspace {
	DevScratch ws, work, srcs, staging, raw, counts, refinedA, refinedB, slot_of, dirs, ndirs, oriented;
	void* pinned = nullptr; size_t pinned_cap = 0;   // host-pinned scratch: source pointer table, counter block
	std::vector<const void*> srcs_last; void* srcs_dev = nullptr;   // the pointer table the device holds (and where)
	long long last_total = 0;                        // descriptors of the previous batch: predicts output capacity
	int last_raw_max = 0, last_refined_max = 0;      // longest per-image lists of the previous batch: size the refine / sort launches
	int raw_cap = 16384;                             // per-image capacity of the raw / refined lists; grows on overflow (run_group)
	int desc_list_cap = OP_DESC_LIST_CAP;            // list arena of the descriptor kernel's sorting pass (op_debug_set_desc_list_cap)
	void release() {
		ws.release(); work.release(); srcs.release(); staging.release(); raw.release(); counts.release();
		refinedA.release(); refinedB.release(); slot_of.release(); dirs.release(); ndirs.release(); oriented.release();
		if (pinned) hipHostFree(pinned); pinned = nullptr; pinned_cap = 0;
		srcs_last.clear(); srcs_dev = nullptr;
	}
};

// Run the whole pipeline for images of one size; ends behind a wait for ctx's stream.  `keep` (staged dump): the working image
// is materialised and the intermediate lists of image 0 go to the host (sift_dump_keep).
int run_group(op_ctx* ctx, CallBlocks& own, const op_config& cfg, const std::vector<const op_image*>& imgs, Workspace& W,
		SiftPlan& plan, FeatArrays& res, op_sift_dump* keep);
// sift_dump.hip: image 0's raw (raw_count), refined (refined_count) and oriented lists and res's descriptors, read behind run_group's wait
int sift_dump_keep(op_sift_dump* keep, const Workspace& W, int cap, const FeatArrays& res, int raw_count, int refined_count);
