// blend_geom.cc -- the O(n) geometry of the blend stage, on the host in fp64 with the host libm exactly like the reference:
// calc_inverse_homo / update_proj_range / get_final_resolution (stitcher_image.cc:36-114), the bounds of
// CylinderProject::project(Shape2D&) (warp.cc:46-67), the multiband blur's taps and the corners and homography of
// CylinderStitcher::perspective_correction (cylstitcher.cc:140-168); and the host parts of the re-projection (the frame of a
// spherical canvas, the view specs, op_canvas_reproject's refusals).  Plain C++ (no HIP), built without contraction;
// tests/harness/photometric_solve_harness.cc, perspective_harness.cc and reproject_harness.cc run it under the sanitizers.
#include "blend_shared.hpp"
#include "ransac_math.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

// ------------------------------- host geometry (fp64, host libm) -------------------------------
// Eigen::FullPivLU 3x3 inverse used by Homography::inverse (stitch/homography.cc:25-39)
bool inverse3_host(const double a[9], double inv[9]) {
	double lu[9]; memcpy(lu, a, sizeof(lu));
	int rowt[3], colt[3], nonzero = 3; double maxpivot = 0;
	for (int k = 0; k < 3; ++k) {
		int br = k, bc = k; double best = -1;
		for (int i = k; i < 3; ++i) for (int j = k; j < 3; ++j) { double v = std::fabs(lu[i * 3 + j]); if (v > best) { best = v; br = i; bc = j; } }
		if (best == 0.0) { nonzero = k; for (int i = k; i < 3; ++i) rowt[i] = colt[i] = i; break; }
		if (best > maxpivot) maxpivot = best;
		rowt[k] = br; colt[k] = bc;
		if (br != k) for (int j = 0; j < 3; ++j) std::swap(lu[k * 3 + j], lu[br * 3 + j]);
		if (bc != k) for (int i = 0; i < 3; ++i) std::swap(lu[i * 3 + k], lu[i * 3 + bc]);
		for (int i = k + 1; i < 3; ++i) lu[i * 3 + k] /= lu[k * 3 + k];
		for (int i = k + 1; i < 3; ++i) for (int j = k + 1; j < 3; ++j) lu[i * 3 + j] -= lu[i * 3 + k] * lu[k * 3 + j];
	}
	const double thr = std::fabs(maxpivot) * (DBL_EPSILON * 3);
	int rank = 0;
	for (int i = 0; i < nonzero; ++i) rank += (std::fabs(lu[i * 3 + i]) > thr);
	if (rank != 3) return false;
	for (int col = 0; col < 3; ++col) {
		double c[3];
		for (int i = 0; i < 3; ++i) c[i] = (i == col) ? 1.0 : 0.0;
		for (int i = 0; i < 3; ++i) std::swap(c[i], c[rowt[i]]);
		for (int i = 0; i < 3; ++i) for (int j = 0; j < i; ++j) c[i] -= lu[i * 3 + j] * c[j];
		for (int i = 2; i >= 0; --i) { for (int j = i + 1; j < 3; ++j) c[i] -= lu[i * 3 + j] * c[j]; c[i] /= lu[i * 3 + i]; }
		for (int i = 2; i >= 0; --i) std::swap(c[i], c[colt[i]]);
		for (int i = 0; i < 3; ++i) inv[i * 3 + col] = c[i];
	}
	return true;
}

void htrans_host(const double* d, double x, double y, double z, double out[3]) {
	out[0] = d[0] * x + d[1] * y + d[2] * z;
	out[1] = d[3] * x + d[4] * y + d[5] * z;
	out[2] = d[6] * x + d[7] * y + d[8] * z;
}
void homo2proj_host(int method, const double h[3], double out[2]) {   // projection.hh:16-18,33-36,48-51
	if (method == 0) { out[0] = h[0] / h[2]; out[1] = h[1] / h[2]; }
	else if (method == 1) { out[0] = std::atan2(h[0], h[2]); out[1] = h[1] / (std::hypot(h[0], h[2])); }
	else { out[0] = std::atan2(h[0], h[2]); out[1] = std::atan2(h[1], std::hypot(h[0], h[2])); }
}

}	// namespace

void roi_of(const op_blend_geom* g, const double* range, int roi[4]) {   // Coor(double, double) truncation
	roi[0] = (int)((range[0] - g->proj_min[0]) / g->resolution[0]);
	roi[1] = (int)((range[1] - g->proj_min[1]) / g->resolution[1]);
	roi[2] = (int)((range[2] - g->proj_min[0]) / g->resolution[0]);
	roi[3] = (int)((range[3] - g->proj_min[1]) / g->resolution[1]);
}

// GaussCache (feature/gaussian.cc:17-40)
int gauss_taps(float sigma, int window_factor, BlurTaps& t) {
	int kw = (int)(std::ceil(0.3 * (sigma / 2 - 1) + 0.8) * window_factor);
	if (kw % 2 == 0) kw++;
	const int center = kw / 2;
	if (center > OP_MAX_KCENTER || kw < 1) return -1;
	float* kernel = &t.k[center];
	kernel[0] = 1;
	float exp_coeff = (float)(-1.0 / (sigma * sigma * 2)), wsum = 1;
	for (int i = 1; i <= center; i++)
		wsum += (kernel[i] = std::exp((float)(i * i) * exp_coeff)) * 2;
	float fac = (float)(1.0 / wsum);
	kernel[0] = fac;
	for (int i = 1; i <= center; i++) kernel[-i] = (kernel[i] *= fac);
	t.center = center;
	return 0;
}

CylProj cyl_projector(int w, int h, double h_factor, float focal_length) {   // warp.cc:70-75
	CylProj p;
	p.r = (int)(std::hypot((double)w, (double)h) * (focal_length / 43.266));
	p.cx = w / 2; p.cy = h / 2 * h_factor;
	p.sizefactor = p.r;
	return p;
}

namespace {

void cyl_proj(const CylProj& P, double px, double py, double out[2]) {       // warp.cc:13-17
	out[0] = std::atan((px - P.cx) / P.r);
	out[1] = (py - P.cy) / (std::hypot(px - P.cx, (double)P.r));
}

}	// namespace

extern "C" {

int op_blend_prepare(const op_config* cfg, int proj_method, int identity_idx, int n, const int* shapes_wh,
		const double* homo, op_blend_geom* g, double* homo_inv, double* ranges) {
	if (!cfg || !shapes_wh || !homo || !g || !homo_inv || !ranges || n <= 0 || identity_idx < 0 || identity_idx >= n ||
			proj_method < 0 || proj_method > 2)
		OP_FAIL(OP_ERR_INVALID, "op_blend_prepare: bad argument");
	for (int i = 0; i < n; ++i)
		if (!inverse3_host(homo + 9 * i, homo_inv + 9 * i))
			OP_FAIL(OP_ERR_INVALID, "op_blend_prepare: homography " + std::to_string(i) + " is not invertible (homography.cc:33)");
	const int CORNER_SAMPLE = 100;        // stitcher_image.cc:43
	std::vector<double> cx, cy;
	for (int i = 0; i < CORNER_SAMPLE; ++i) {
		const double xi = (double)i / CORNER_SAMPLE - 0.5;
		cx.push_back(xi); cy.push_back(-0.5);
		cx.push_back(xi); cy.push_back(0.5);
	}
	for (int j = 0; j < CORNER_SAMPLE; ++j) {
		const double yj = (double)j / CORNER_SAMPLE - 0.5;
		cx.push_back(-0.5); cy.push_back(yj);
		cx.push_back(0.5); cy.push_back(yj);
	}
	double pmin[2] = {DBL_MAX, DBL_MAX}, pmax[2] = {-DBL_MAX, -DBL_MAX};
	for (int m = 0; m < n; ++m) {
		const int w = shapes_wh[2 * m], h = shapes_wh[2 * m + 1];
		double nmin[2] = {DBL_MAX, DBL_MAX}, nmax[2] = {-DBL_MAX, -DBL_MAX};
		for (size_t k = 0; k < cx.size(); ++k) {
			double hv[3], t[2];
			htrans_host(homo + 9 * m, cx[k] * w, cy[k] * h, 1, hv);
			homo2proj_host(proj_method, hv, t);
			for (int c = 0; c < 2; ++c) { if (t[c] < nmin[c]) nmin[c] = t[c]; if (nmax[c] < t[c]) nmax[c] = t[c]; }
		}
		ranges[4 * m] = nmin[0]; ranges[4 * m + 1] = nmin[1]; ranges[4 * m + 2] = nmax[0]; ranges[4 * m + 3] = nmax[1];
		for (int c = 0; c < 2; ++c) { if (nmin[c] < pmin[c]) pmin[c] = nmin[c]; if (pmax[c] < nmax[c]) pmax[c] = nmax[c]; }
	}
	g->proj_method = proj_method;
	g->proj_min[0] = pmin[0]; g->proj_min[1] = pmin[1]; g->proj_max[0] = pmax[0]; g->proj_max[1] = pmax[1];
	// get_final_resolution (stitcher_image.cc:79-114)
	const int refw = shapes_wh[2 * identity_idx], refh = shapes_wh[2 * identity_idx + 1];
	double c2[3], c1[3], p2[2], p1[2];
	htrans_host(homo + 9 * identity_idx, refw / 2.0, refh / 2.0, 1, c2);
	htrans_host(homo + 9 * identity_idx, -refw / 2.0, -refh / 2.0, 1, c1);
	homo2proj_host(proj_method, c2, p2); homo2proj_host(proj_method, c1, p1);
	double rx = p2[0] - p1[0], ry = p2[1] - p1[1];
	if (proj_method != 0) {
		if (rx < 0) rx = 2 * M_PI + rx;
		if (ry < 0) ry = M_PI + ry;
	}
	double resx = std::fabs(rx) / (double)refw, resy = std::fabs(ry) / (double)refh;
	const double tsx = (pmax[0] - pmin[0]) / resx, tsy = (pmax[1] - pmin[1]) / resy;
	const double max_edge = std::max(tsx, tsy);
	if (max_edge > 80000 || tsx * tsy > 1e9)
		OP_FAIL(OP_ERR_INVALID, "Target size too large. Looks like a stitching failure!");   // stitcher_image.cc:105-106
	if (max_edge > cfg->MAX_OUTPUT_SIZE) {
		const float ratio = (float)(max_edge / cfg->MAX_OUTPUT_SIZE);
		resx *= ratio; resy *= ratio;
	}
	g->resolution[0] = resx; g->resolution[1] = resy;
	return OP_OK;
}

int op_blend_canvas_dims(const op_blend_geom* g, const op_blend_image* imgs, int n, int* h, int* w) {
	if (!g || !imgs || n <= 0 || !h || !w) OP_FAIL(OP_ERR_INVALID, "op_blend_canvas_dims: bad argument");
	int tx = 0, ty = 0;       // Coor target_size{0,0}; update_max(bottom_right) (blender.cc:21)
	for (int i = 0; i < n; ++i) {
		int roi[4]; roi_of(g, imgs[i].range, roi);
		tx = std::max(tx, roi[2]); ty = std::max(ty, roi[3]);
	}
	*h = ty; *w = tx;
	return OP_OK;
}

int op_cyl_warp_shape(const op_config* cfg, int w, int h, double h_factor, double* pts, int npts,
		int* new_w, int* new_h, double* offset) {
	if (!cfg || w < 2 || h < 2 || npts < 0 || (npts && !pts) || !new_w || !new_h || !offset)
		OP_FAIL(OP_ERR_INVALID, "op_cyl_warp_shape: bad argument");
	const CylProj P = cyl_projector(w, h, h_factor, cfg->FOCAL_LENGTH);
	if (P.r <= 0) OP_FAIL(OP_ERR_INVALID, "op_cyl_warp_shape: degenerate projector radius");
	// warp.cc:47-52 scans all w*h pixels.  x = atan((j-cx)/r) does not depend on i, and for a fixed
	// j the quotient y = (i-cy)/hypot(j-cx, r) is monotone in i in floating point as well (one
	// subtraction and one division by a fixed positive number), so rows 0 and h-1 hold both
	// extremes of every column: 2w evaluations give the identical min/max.
	double mn[2] = {DBL_MAX, DBL_MAX}, mx[2] = {0, 0};
	for (int j = 0; j < w; ++j) for (int e = 0; e < 2; ++e) {
		double c[2]; cyl_proj(P, j, e ? h - 1 : 0, c);
		for (int q = 0; q < 2; ++q) { if (c[q] < mn[q]) mn[q] = c[q]; if (mx[q] < c[q]) mx[q] = c[q]; }
	}
	for (int q = 0; q < 2; ++q) { mx[q] = mx[q] * P.sizefactor; mn[q] = mn[q] * P.sizefactor; }
	const double rsx = mx[0] - mn[0], rsy = mx[1] - mn[1];
	offset[0] = mn[0] * (-1); offset[1] = mn[1] * (-1);
	const int sx = (int)rsx, sy = (int)rsy;
	for (int k = 0; k < npts; ++k) {              // warp.cc:59-65
		double c[2];
		cyl_proj(P, pts[2 * k] + w / 2, pts[2 * k + 1] + h / 2, c);
		pts[2 * k] = c[0] * P.sizefactor + offset[0];
		pts[2 * k + 1] = c[1] * P.sizefactor + offset[1];
		pts[2 * k] -= sx / 2;
		pts[2 * k + 1] -= sy / 2;
	}
	*new_w = sx; *new_h = sy;
	return OP_OK;
}

// CylinderStitcher::perspective_correction's geometry (cylstitcher.cc:140-168)
int op_perspective_homography(const op_blend_geom* g, int ref_w, int ref_h, int first_w, int first_h, const double* first_homo,
		int last_w, int last_h, const double* last_homo, int canvas_w, int canvas_h, double* inv, double* corners) {
	if (!g || !first_homo || !last_homo || !inv) OP_FAIL(OP_ERR_INVALID, "op_perspective_homography: bad argument");
	if (ref_w < 1 || ref_h < 1 || first_w < 1 || first_h < 1 || last_w < 1 || last_h < 1 || canvas_w < 1 || canvas_h < 1)
		OP_FAIL(OP_ERR_INVALID, "op_perspective_homography: a size below 1");
	const int refw = ref_w, refh = ref_h;
	opransac::P2 cor[4];
	auto to_ref_coor = [&](int k, const double* homo, int w, int h, double vx, double vy) {    // :148-156
		vx *= w; vy *= h;
		double hv[3], t[2];
		htrans_host(homo, vx, vy, 1, hv);
		hv[0] /= refw; hv[1] /= refh;
		homo2proj_host(0, hv, t);                       // proj_method is flat by now (:25)
		t[0] *= refw; t[1] *= refh;
		cor[k].x = t[0] - g->proj_min[0]; cor[k].y = t[1] - g->proj_min[1];
	};
	to_ref_coor(0, first_homo, first_w, first_h, -0.5, -0.5);
	to_ref_coor(1, first_homo, first_w, first_h, -0.5, 0.5);
	to_ref_coor(2, last_homo, last_w, last_h, 0.5, -0.5);
	to_ref_coor(3, last_homo, last_w, last_h, 0.5, 0.5);
	if (corners) for (int k = 0; k < 4; ++k) { corners[2 * k] = cor[k].x; corners[2 * k + 1] = cor[k].y; }
	for (int k = 0; k < 4; ++k)
		if (!std::isfinite(cor[k].x) || !std::isfinite(cor[k].y)) OP_FAIL(OP_ERR_INVALID, "op_perspective_homography: a corner is not finite");
	// Four points of which three lie on one line are the image of a rectangle under no homography: the 8 x 8 system is
	// singular there, and the solver below would drop the direction and return some finite matrix.
	for (int k = 0; k < 4; ++k) {
		const opransac::P2 a = cor[k], b = cor[(k + 1) & 3], c = cor[(k + 2) & 3];
		const double ux = b.x - a.x, uy = b.y - a.y, vx = c.x - a.x, vy = c.y - a.y;
		if (std::fabs(ux * vy - uy * vx) <= 1e-12 * std::sqrt(ux * ux + uy * uy) * std::sqrt(vx * vx + vy * vy))
			OP_FAIL(OP_ERR_INVALID, "op_perspective_homography: three corners on one line");
	}
	// corners_std (:164-166) and getPerspectiveTransform(corners, corners_std) (:167): from the canvas rectangle onto the corners
	const opransac::P2 std_[4] = {{0, 0}, {0, (double)canvas_h}, {(double)canvas_w, 0}, {(double)canvas_w, (double)canvas_h}};
	double H[9];
	opransac::calc_transform(4, [&](int i) { return cor[i]; }, [&](int i) { return std_[i]; }, false, H);
	for (int k = 0; k < 9; ++k) if (!std::isfinite(H[k])) OP_FAIL(OP_ERR_INVALID, "op_perspective_homography: the homography is not finite");
	memcpy(inv, H, sizeof(H));
	return OP_OK;
}

// ---- the host parts of the re-projection (reproject.hip): where a spherical canvas sits, and the view specs ----
int op_pano_frame_of(const op_blend_geom* g, int x0, int y0, op_pano_frame* f) {
	if (!g || !f) OP_FAIL(OP_ERR_INVALID, "op_pano_frame_of: bad argument");
	if (g->proj_method != 2) OP_FAIL(OP_ERR_UNSUPPORTED, "op_pano_frame_of: the canvas is not spherical");
	f->lon0 = g->proj_min[0] + (double)x0 * g->resolution[0];
	f->lat0 = g->proj_min[1] + (double)y0 * g->resolution[1];
	f->step_lon = g->resolution[0]; f->step_lat = g->resolution[1];
	f->wrap = 0;
	return OP_OK;
}

int op_view_look(double yaw, double pitch, double roll, double hfov, int out_w, int out_h, op_view_spec* s) {
	if (!s) OP_FAIL(OP_ERR_INVALID, "op_view_look: bad argument");
	if (!std::isfinite(yaw) || !std::isfinite(pitch) || !std::isfinite(roll)) OP_FAIL(OP_ERR_INVALID, "op_view_look: an angle is not finite");
	if (!(hfov > 0 && hfov < M_PI)) OP_FAIL(OP_ERR_INVALID, "op_view_look: hfov outside (0, pi)");
	if (out_w < 1 || out_h < 1) OP_FAIL(OP_ERR_INVALID, "op_view_look: a size below 1");
	const double cy = std::cos(yaw), sy = std::sin(yaw), cp = std::cos(pitch), sp = std::sin(pitch), cr = std::cos(roll), sr = std::sin(roll);
	const double Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cp, -sp, 0, sp, cp}, Rz[9] = {cr, -sr, 0, sr, cr, 0, 0, 0, 1};
	double A[9];
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i * 3 + j] = Ry[i * 3] * Rx[j] + Ry[i * 3 + 1] * Rx[3 + j] + Ry[i * 3 + 2] * Rx[6 + j];
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) s->rot[i * 3 + j] = A[i * 3] * Rz[j] + A[i * 3 + 1] * Rz[3 + j] + A[i * 3 + 2] * Rz[6 + j];
	s->mode = OP_VIEW_RECTILINEAR; s->out_h = out_h; s->out_w = out_w;
	s->focal = 0.5 * (double)out_w / std::tan(0.5 * hfov);
	return OP_OK;
}

int op_view_cube_face(int face, int n, op_view_spec* s) {
	if (!s || face < 0 || face > 5 || n < 1) OP_FAIL(OP_ERR_INVALID, "op_view_cube_face: bad argument");
	// columns: where the picture's right, down and forward point (include/openpano_hip.h names each face's top)
	static const double R[6][9] = {
		{0, 0, 1, 0, 1, 0, -1, 0, 0},      // +x: right -z, down +y
		{0, 0, -1, 0, 1, 0, 1, 0, 0},      // -x: right +z, down +y
		{1, 0, 0, 0, 0, 1, 0, -1, 0},      // +y: right +x, down -z
		{1, 0, 0, 0, 0, -1, 0, 1, 0},      // -y: right +x, down +z
		{1, 0, 0, 0, 1, 0, 0, 0, 1},       // +z: right +x, down +y
		{-1, 0, 0, 0, 1, 0, 0, 0, -1}};    // -z: right -x, down +y
	memcpy(s->rot, R[face], sizeof(s->rot));
	s->mode = OP_VIEW_RECTILINEAR; s->out_h = n; s->out_w = n; s->focal = 0.5 * (double)n;
	return OP_OK;
}

int op_view_planet(int n, op_view_spec* s) {
	if (!s || n < 1) OP_FAIL(OP_ERR_INVALID, "op_view_planet: bad argument");
	static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	memcpy(s->rot, I, sizeof(s->rot));
	s->mode = OP_VIEW_PLANET; s->out_h = n; s->out_w = n; s->focal = 1.0;
	return OP_OK;
}

}	// extern "C"

// op_canvas_reproject's refusals, here so that the sanitizer program reaches them without a device
int reproject_check(const op_pano_frame* f, const op_view_spec* s) {
	if (!f || !s) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: bad argument");
	if (s->mode != OP_VIEW_PLANET && s->mode != OP_VIEW_RECTILINEAR) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: unknown mode " + std::to_string(s->mode));
	if (s->out_h < 1 || s->out_w < 1) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: a size below 1");
	if (s->mode == OP_VIEW_PLANET && s->out_h != s->out_w) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: a planet is square");
	bool finite = std::isfinite(f->lon0) && std::isfinite(f->lat0) && std::isfinite(f->step_lon) && std::isfinite(f->step_lat) && std::isfinite(s->focal);
	for (int k = 0; k < 9; ++k) finite = finite && std::isfinite(s->rot[k]);
	if (!finite) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: a field is not finite");
	if (!(s->focal > 0)) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: focal is not positive");
	if (f->wrap != 0 && f->wrap != 1) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: wrap is neither 0 nor 1");
	if (f->step_lat == 0 || (!f->wrap && f->step_lon == 0)) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: a step is zero");
	if (f->wrap && !(f->lon0 >= -M_PI && f->lon0 <= M_PI)) OP_FAIL(OP_ERR_INVALID, "op_canvas_reproject: wrap with lon0 outside [-pi, pi]");
	return OP_OK;
}
