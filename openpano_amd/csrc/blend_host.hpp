// blend_host.hpp -- the host set-up that the blend (blend.hip, where the three are defined) and the overlap statistics
// (overlap.hip) share: the images as BlendImg on the device, the geometry checks, the canvas map's trig tables.
#pragma once
#include "blend_sample.hpp"

int upload_images(op_ctx* ctx, const char* who, const op_blend_geom* g, const op_blend_image* imgs, int n, CallBlocks& own,
		std::vector<BlendImg>& h_imgs, long long& roi_total, long long& max_roi, bool& any_u8, BlendImg** d_out);
int check_blend_args(const char* who, const op_blend_geom* g);
hipError_t trig_tables(op_ctx* ctx, const BlendGeom& g, int w1, int h1, BlendTrig* out);
