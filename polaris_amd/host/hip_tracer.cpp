#include "hip_tracer.hpp"

#include <cmath>
#include <cstring>

// The C ABI's polaris_hip_set_lens, referenced weakly: this file is also linked against stand-ins of the C ABI that know no lens
// (tests/tools/mock_polaris_hip.cpp); there a CameraData with a lens is refused and one without asks nothing.
extern "C" int polaris_hip_set_lens(polaris_hip_tracer *h, const PolarisLensParams *p) __attribute__((weak));
// polaris_hip_set_shutter likewise: without it only a CameraData that has a close state is refused.
extern "C" int polaris_hip_set_shutter(polaris_hip_tracer *h, const PolarisShutterParams *p) __attribute__((weak));
// polaris_hip_set_projection likewise: without it only a CameraData that has a projection is refused.
extern "C" int polaris_hip_set_projection(polaris_hip_tracer *h, const PolarisProjectionParams *p) __attribute__((weak));

namespace polaris {
namespace tracer {
namespace hip {

using clock_ = std::chrono::steady_clock;

std::vector<Device> Devices(const std::vector<std::string> &blacklist) { // renderer/default.go:204-224
	std::vector<Device> out;
	const int n = polaris_hip_device_count();
	for (int i = 0; i < n; i++) {
		char name[256] = {0};
		uint32_t cus = 0, mhz = 0;
		uint64_t mem = 0;
		if (polaris_hip_device_info(i, name, &cus, &mhz, &mem) != POLARIS_OK) continue;
		Device d{i, name, cus * mhz / 1000};
		bool skip = false;
		for (const auto &b : blacklist)
			if (!b.empty() && d.Name.find(b) != std::string::npos) skip = true;
		if (!skip) out.push_back(d);
	}
	return out;
}

HipTracer::HipTracer(std::string id, Device dev, SeedSource seeds) : id_(std::move(id)), dev_(std::move(dev)), seeds_(std::move(seeds)) {}
HipTracer::~HipTracer() { Close(); }

Error HipTracer::check(int rc) {
	if (rc == POLARIS_OK) return Error::Nil();
	const char *m = polaris_hip_last_error(h_);
	return Error{rc, std::string("hip tracer (") + dev_.Name + "): " + (m ? m : "")};
}

// The lens vectors of a CameraData (polaris_amd/ctypes_api.py lens_from_frustum, the same derivation): axis = normalize(TL + TR + BL +
// BR), u = radius normalize(TR - TL), v = radius normalize(TL - BL), in double, rounded to float once.  lens_radius = 0: all zero (off).
static PolarisLensParams lensFromFrustum(const float *frustum, float lens_radius, float focus_distance) {
	PolarisLensParams p{};
	p.struct_size = sizeof p;
	if (lens_radius == 0.0f) return p;
	p.focus_distance = focus_distance;
	const float *tl = frustum, *tr = frustum + 4, *bl = frustum + 8, *br = frustum + 12;
	double a[3], u[3], v[3];
	for (int k = 0; k < 3; k++) {
		a[k] = (((double)tl[k] + (double)tr[k]) + (double)bl[k]) + (double)br[k];
		u[k] = (double)tr[k] - (double)tl[k];
		v[k] = (double)tl[k] - (double)bl[k];
	}
	auto unit = [](double x[3]) { const double n = std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); for (int k = 0; k < 3; k++) x[k] = x[k] / n; };
	unit(a); unit(u); unit(v);
	for (int k = 0; k < 3; k++) { p.axis[k] = (float)a[k]; p.u[k] = (float)((double)lens_radius * u[k]); p.v[k] = (float)((double)lens_radius * v[k]); }
	return p;
}

// The shutter of a CameraData: off without a close state; else the close camera, and under a lens the close lens -- the vectors of
// frustum1 with the same radius, focused at focus_distance1 (polaris_amd/tracer.py set_shutter, the same derivation).
static PolarisShutterParams shutterOf(const CameraData &c) {
	PolarisShutterParams p{};
	p.struct_size = sizeof p;
	if (!c.has_close) return p;
	p.enabled = 1;
	memcpy(p.eye1, c.eye1, sizeof p.eye1);
	memcpy(p.frustum1, c.frustum1, sizeof p.frustum1);
	const PolarisLensParams l = lensFromFrustum(c.frustum1, c.lens_radius, c.focus_distance1 > 0.0f ? c.focus_distance1 : c.focus_distance);
	p.focus_distance1 = l.focus_distance;
	memcpy(p.axis1, l.axis, sizeof p.axis1); memcpy(p.u1, l.u, sizeof p.u1); memcpy(p.v1, l.v, sizeof p.v1);
	return p;
}

// The projection of a CameraData (polaris_amd/ctypes_api.py projection_for, the same derivation): axis = normalize(TL + TR + BL + BR),
// right = normalize(TR - TL), up = normalize(TL - BL) made orthogonal to the axis, half_height = ortho_height / 2, half_width =
// half_height |TR - TL| / |TL - BL|, in double, rounded to float once.  projection = 0: all zero (off).
static PolarisProjectionParams projectionOf(const CameraData &c) {
	PolarisProjectionParams p{};
	p.struct_size = sizeof p;
	if (c.projection == POLARIS_PROJECTION_PERSPECTIVE) return p;
	p.kind = c.projection;
	const float *tl = c.frustum, *tr = c.frustum + 4, *bl = c.frustum + 8, *br = c.frustum + 12;
	double a[3], r[3], u[3];
	for (int k = 0; k < 3; k++) {
		a[k] = (((double)tl[k] + (double)tr[k]) + (double)bl[k]) + (double)br[k];
		r[k] = (double)tr[k] - (double)tl[k];
		u[k] = (double)tl[k] - (double)bl[k];
	}
	auto length = [](const double x[3]) { return std::sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); };
	const double la = length(a), lr = length(r), lu = length(u);
	for (int k = 0; k < 3; k++) { a[k] = a[k] / la; r[k] = r[k] / lr; u[k] = u[k] / lu; }
	const double ua = (u[0] * a[0] + u[1] * a[1]) + u[2] * a[2];
	for (int k = 0; k < 3; k++) u[k] = u[k] - a[k] * ua;
	const double lu2 = length(u);
	for (int k = 0; k < 3; k++) { p.axis[k] = (float)a[k]; p.right[k] = (float)r[k]; p.up[k] = (float)(u[k] / lu2); }
	if (c.projection == POLARIS_PROJECTION_ORTHOGRAPHIC) {
		const double half_height = (double)c.ortho_height / 2.0;
		p.half_height = (float)half_height;
		p.half_width = (float)(half_height * (lr / lu));
	} else {
		p.lon_range = c.lon_range;
		p.lat_range = c.lat_range;
	}
	return p;
}

Error HipTracer::Init() {
	std::lock_guard<std::mutex> lk(mu_);
	return check(polaris_hip_create(dev_.Index, &h_));
}

void HipTracer::Close() {
	std::lock_guard<std::mutex> lk(mu_);
	if (h_) polaris_hip_destroy(h_);
	h_ = nullptr;
}

Error HipTracer::UpdateState(UpdateMode mode, ChangeType type, const void *data, Duration *took) {
	{
		std::lock_guard<std::mutex> lk(change_mu_);
		switch (type) {
		case ChangeType::FrameDimensions: dims_ = *static_cast<const FrameDims *>(data); has_dims_ = true; break;
		case ChangeType::SceneData: scene_ = static_cast<const PolarisSceneView *>(data); has_scene_ = true; break;
		case ChangeType::CameraData: cam_ = *static_cast<const CameraData *>(data); has_cam_ = true; break;
		default: return Error{POLARIS_E_BAD_ARGUMENT, "unsupported change type"};
		}
	}
	if (mode == UpdateMode::Synchronous) return commitChanges(took);
	if (took) *took = Duration{0};
	return Error::Nil();
}

Error HipTracer::commitChanges(Duration *took) { // tracer/opencl/tracer.go:161-192
	const auto start = clock_::now();
	std::lock_guard<std::mutex> lk(change_mu_);
	Error err;
	if (has_dims_ && !err) { err = check(polaris_hip_resize(h_, dims_.w, dims_.h)); has_dims_ = false; }
	if (has_scene_ && !err) { err = check(polaris_hip_upload_scene(h_, scene_)); has_scene_ = false; scene_ = nullptr; }
	if (has_cam_ && !err) {
		err = check(polaris_hip_set_camera(h_, cam_.eye, cam_.frustum));
		// the projection excludes the lens and the shutter: one that goes off goes before they may come on, one that is on comes after them
		const PolarisProjectionParams projection = projectionOf(cam_);
		if (!err && polaris_hip_set_projection && projection.kind == POLARIS_PROJECTION_PERSPECTIVE) err = check(polaris_hip_set_projection(h_, &projection));
		// set_camera leaves the lens vectors alone: they follow the new frustum here (identical bytes ask nothing of the library)
		const PolarisLensParams lens = lensFromFrustum(cam_.frustum, cam_.lens_radius, cam_.focus_distance);
		if (!err && polaris_hip_set_lens) err = check(polaris_hip_set_lens(h_, &lens));
		else if (!err && cam_.lens_radius != 0.0f) err = Error{POLARIS_E_BAD_ARGUMENT, "hip tracer: this C ABI has no polaris_hip_set_lens"};
		// camera, lens, then shutter: set_camera has switched it off, so a CameraData without a close state asks nothing more
		const PolarisShutterParams shutter = shutterOf(cam_);
		if (!err && polaris_hip_set_shutter) err = check(polaris_hip_set_shutter(h_, &shutter));
		else if (!err && cam_.has_close) err = Error{POLARIS_E_BAD_ARGUMENT, "hip tracer: this C ABI has no polaris_hip_set_shutter"};
		// camera, then projection: set_camera keeps the projection's basis, which follows the new frustum here (identical bytes ask nothing)
		if (!err && projection.kind != POLARIS_PROJECTION_PERSPECTIVE) {
			if (polaris_hip_set_projection) err = check(polaris_hip_set_projection(h_, &projection));
			else err = Error{POLARIS_E_BAD_ARGUMENT, "hip tracer: this C ABI has no polaris_hip_set_projection"};
		}
		has_cam_ = false;
	}
	stats_.UpdateTime = std::chrono::duration_cast<Duration>(clock_::now() - start);
	if (took) *took = stats_.UpdateTime;
	return err;
}

Error HipTracer::Trace(BlockRequest *req, Duration *took) { // tracer/opencl/tracer.go:194-247
	const auto start = clock_::now();
	if (Error e = commitChanges(nullptr)) return e;
	const size_t stride = 1 + req->num_bounces;
	std::vector<uint32_t> seeds((size_t)req->samples_per_pixel * stride);
	for (uint32_t s = 0; s < req->samples_per_pixel; s++) { // same draw order as the reference
		req->seed = seeds_();
		seeds[s * stride] = req->seed;
		for (uint32_t b = 0; b < req->num_bounces; b++) seeds[s * stride + 1 + b] = seeds_();
	}
	if (Error e = check(polaris_hip_trace(h_, req, seeds.data(), seeds.size(), &last_))) return e;
	req->accumulated_samples += req->samples_per_pixel; // tracer.go:240
	stats_.BlockW = req->block_w;
	stats_.BlockH = req->block_h;
	stats_.RenderTime = std::chrono::duration_cast<Duration>(clock_::now() - start);
	if (took) *took = stats_.RenderTime;
	return Error::Nil();
}

Error HipTracer::MergeOutput(Tracer *other, BlockRequest *req, Duration *took) { // tracer.go:279-286
	const auto start = clock_::now();
	auto *src = dynamic_cast<HipTracer *>(other);
	if (!src) return Error{POLARIS_E_UNSUPPORTED, "merge failed: unsupported tracer instance"};
	Error e = check(polaris_hip_merge(h_, src->h_, req));
	if (took) *took = std::chrono::duration_cast<Duration>(clock_::now() - start);
	return e;
}

Error HipTracer::SyncFramebuffer(BlockRequest *req, Duration *took) { // tracer.go:250-276
	const auto start = clock_::now();
	Error e = check(polaris_hip_sync_framebuffer(h_, req));
	if (took) *took = std::chrono::duration_cast<Duration>(clock_::now() - start);
	return e;
}

Error HipTracer::ReadFrameBuffer(uint8_t *rgba, size_t n) { return check(polaris_hip_read_framebuffer(h_, rgba, n)); }
Error HipTracer::ReadAccumulator(int which, float *out, size_t n) { return check(polaris_hip_read_accumulator(h_, which, out, n)); }

} // namespace hip
} // namespace tracer
} // namespace polaris
