// ctx.hip — context, error reporting, device-memory helpers, projection batch (a8/a12/a13).
#include <chrono>
#include <cstdarg>

#include "common.h"

static thread_local char g_err[512] = "";

void ptam_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int ctx_scratch(ptam_ctx* ctx, size_t bytes, void** out) {
    if (bytes > ctx->d_scratch_cap) {
        HIP_TRY(ptam_stream_wait(ctx->stream));
        if (ctx->d_scratch) HIP_TRY(hipFree(ctx->d_scratch));
        ctx->d_scratch = nullptr;
        ctx->d_scratch_cap = 0;
        size_t cap = bytes + bytes / 2 + 4096;
        HIP_TRY(hipMalloc(&ctx->d_scratch, cap));
        ctx->d_scratch_cap = cap;
    }
    *out = ctx->d_scratch;
    return PTAM_OK;
}

void ptam_preload(const void* kernel) {
    hipFuncAttributes a;
    if (hipFuncGetAttributes(&a, kernel) != hipSuccess) (void)hipGetLastError();
}

hipError_t ptam_stream_wait(hipStream_t stream) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(stream);
        if (q != hipErrorNotReady) return q;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    (void)hipGetLastError();   // (hipErrorNotReady is sticky in the last-error slot)
    return hipStreamSynchronize(stream);
}

static ptam_ctx::Cached* ctx_cache_of(ptam_ctx* ctx, CtxMem kind, int* slots) {
    switch (kind) {
        case CTX_MEM_DEVICE: *slots = CTX_NCACHE(ctx->dev_cache); return ctx->dev_cache;
        case CTX_MEM_PINNED: *slots = CTX_NCACHE(ctx->pin_cache); return ctx->pin_cache;
        default: *slots = CTX_NCACHE(ctx->host_cache); return ctx->host_cache;
    }
}
int ctx_block_take(ptam_ctx* ctx, CtxMem kind, size_t bytes, void** out, size_t* cap) {
    int slots = 0, best = -1;
    ptam_ctx::Cached* c = ctx_cache_of(ctx, kind, &slots);
    for (int i = 0; i < slots; i++)   // the smallest released block that fits
        if (c[i].p && c[i].bytes >= bytes && (best < 0 || c[i].bytes < c[best].bytes)) best = i;
    if (best >= 0) {
        *out = c[best].p;
        *cap = c[best].bytes;
        c[best].p = nullptr;
        c[best].bytes = 0;
        return PTAM_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (kind == CTX_MEM_DEVICE)
        HIP_TRY(hipMalloc(out, bytes));
    else
        HIP_TRY(hipHostMalloc(out, bytes, kind == CTX_MEM_PINNED ? hipHostMallocDefault : hipHostMallocMapped | hipHostMallocCoherent));
    *cap = bytes;
    return PTAM_OK;
}
void ctx_block_give(ptam_ctx* ctx, CtxMem kind, void* p, size_t cap) {
    if (!p) return;
    int slots = 0, small = 0;
    ptam_ctx::Cached* c = ctx_cache_of(ctx, kind, &slots);
    for (int i = 0; i < slots; i++)
        if (!c[i].p) {
            c[i].p = p;
            c[i].bytes = cap;
            return;
        }
    for (int i = 1; i < slots; i++)   // every slot taken: keep the largest
        if (c[i].bytes < c[small].bytes) small = i;
    if (cap > c[small].bytes) {
        std::swap(p, c[small].p);
        c[small].bytes = cap;
    }
    if (kind == CTX_MEM_DEVICE)
        hipFree(p);
    else
        hipHostFree(p);
}

int ctx_pinned(ptam_ctx* ctx, size_t bytes, void** out) {
    if (bytes > ctx->h_pinned_cap) {
        HIP_TRY(ptam_stream_wait(ctx->stream));
        if (ctx->h_pinned) HIP_TRY(hipHostFree(ctx->h_pinned));
        ctx->h_pinned = nullptr;
        ctx->h_pinned_cap = 0;
        size_t cap = bytes + bytes / 2 + 4096;
        HIP_TRY(hipHostMalloc(&ctx->h_pinned, cap, hipHostMallocMapped | hipHostMallocCoherent));
        ctx->h_pinned_cap = cap;
        std::memset(ctx->h_pinned, 0, cap);
        HIP_TRY(hipHostGetDevicePointer(&ctx->d_pinned, ctx->h_pinned, 0));
    }
    *out = ctx->h_pinned;
    return PTAM_OK;
}

// RefreshParams src/ATANCamera.cc:27-66 (only the members the hot path reads): devcam_refresh, common.h
static DevCam make_devcam(const ptam_cam_params& p) { return devcam_refresh(p.width, p.height, p.fx, p.fy, p.cx, p.cy, p.w); }

// TrackerData::Project + GetProjectionDerivs (include/Tracker.h:70-94)
__global__ void project_points_kernel(DevCam cam, int n, const double* __restrict__ world,
                                      const double* __restrict__ pose, ptam_projection* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = pose[k];
    ptam_projection p;
    p.image[0] = p.image[1] = 0;
    p.derivs[0] = p.derivs[1] = p.derivs[2] = p.derivs[3] = 0;
    p.in_image = 0;
    p.pad_ = 0;
    se3_apply(T, world[3 * i], world[3 * i + 1], world[3 * i + 2], p.cam[0], p.cam[1], p.cam[2]);
    if (!(p.cam[2] < 0.001)) {
        const double x = p.cam[0] / p.cam[2], y = p.cam[1] / p.cam[2];
        if (!(x * x + y * y > cam.largest_radius * cam.largest_radius)) {
            double u, v, r, f;
            cam_project(cam, x, y, u, v, r, f);
            p.image[0] = u;
            p.image[1] = v;
            cam_derivs(cam, x, y, r, f, p.derivs);
            const bool invalid = r > cam.max_r;
            if (!invalid && !(u < 0 || v < 0 || u > cam.width || v > cam.height)) p.in_image = 1;
        }
    }
    out[i] = p;
}

// TrackerData::Project on existing state (include/Tracker.h:70-85): v3Cam always, v2Image once the camera model is reached,
// m2CamDerivs untouched (ProjectAndDerivs only refreshes them for found points, :89-94)
__global__ void reproject_points_kernel(DevCam cam, int n, const double* __restrict__ world, const double* __restrict__ pose,
                                        ptam_projection* __restrict__ io) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = pose[k];
    ptam_projection p = io[i];
    p.in_image = 0;
    se3_apply(T, world[3 * i], world[3 * i + 1], world[3 * i + 2], p.cam[0], p.cam[1], p.cam[2]);
    if (!(p.cam[2] < 0.001)) {
        const double x = p.cam[0] / p.cam[2], y = p.cam[1] / p.cam[2];
        if (!(x * x + y * y > cam.largest_radius * cam.largest_radius)) {
            double u, v, r, f;
            cam_project(cam, x, y, u, v, r, f);
            p.image[0] = u;
            p.image[1] = v;
            if (!(r > cam.max_r) && !(u < 0 || v < 0 || u > cam.width || v > cam.height)) p.in_image = 1;
        }
    }
    io[i] = p;
}

extern "C" {

const char* ptam_last_error(void) { return g_err; }

int ptam_device_count(int* n) {
    ARG_TRY(n);
    HIP_TRY(hipGetDeviceCount(n));
    return PTAM_OK;
}

int ptam_ctx_create(const ptam_cam_params* cam, int device, ptam_ctx** out) {
    ARG_TRY(cam && out);
    ARG_TRY(cam->width > 0 && cam->height > 0 && cam->fx != 0 && cam->fy != 0);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0 || device < 0 || device >= ndev) {
        ptam_set_error("no HIP device %d (count %d): libptam_hip has no CPU fallback", device, ndev);
        return PTAM_E_HIP;
    }
    HIP_TRY(hipSetDevice(device));
    ptam_ctx* c = new ptam_ctx();
    std::memset(c, 0, sizeof *c);
    c->device = device;
    c->params = *cam;
    c->cam = make_devcam(*cam);
    c->halfsample = PTAM_HALFSAMPLE_R;
    {
        hipDeviceProp_t prop;
        c->n_cu = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
    }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        ptam_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        delete c;
        return PTAM_E_HIP;
    }
    ptam_preload((const void*)project_points_kernel);
    ptam_preload((const void*)reproject_points_kernel);
    trackmap_preload_kernels();
    refind_preload_kernels();
    maprefind_preload_kernels();
    maptables_preload_kernels();
    maprmap_preload_kernels();
    maprmap_keyframe_preload_kernels();
    maprmap_publish_preload_kernels();
    maprmap_init_preload_kernels();
    framereport_preload_kernels();
    tracker_run_preload_kernels();
    if (const int rc = ba_preload_kernels()) {   // (its error text stands)
        hipStreamDestroy(c->stream);
        delete c;
        return rc;
    }
    solve_preload_kernels();
    pose_preload_kernels();
    patch_preload_kernels();
    mapmaker_preload_kernels();
    trails_preload_kernels();
    homography_preload_kernels();
    mapba_preload_kernels();
    mapalign_preload_kernels();
    kf_preload_kernels();
    pvs_preload_kernels();
    sbi_preload_kernels();
    calib_preload_kernels();
    *out = c;
    return PTAM_OK;
}

int ptam_ctx_destroy(ptam_ctx* ctx) {
    if (!ctx) return PTAM_OK;
    hipSetDevice(ctx->device);
    ptam_stream_wait(ctx->stream);
    if (ctx->d_scratch) hipFree(ctx->d_scratch);
    if (ctx->h_pinned) hipHostFree(ctx->h_pinned);
    for (int i = 0; i < CTX_NCACHE(ctx->dev_cache); i++)
        if (ctx->dev_cache[i].p) hipFree(ctx->dev_cache[i].p);
    for (int i = 0; i < CTX_NCACHE(ctx->host_cache); i++)
        if (ctx->host_cache[i].p) hipHostFree(ctx->host_cache[i].p);
    for (int i = 0; i < CTX_NCACHE(ctx->pin_cache); i++)
        if (ctx->pin_cache[i].p) hipHostFree(ctx->pin_cache[i].p);
    if (ctx->d_smap) hipFree(ctx->d_smap);
    hipStreamDestroy(ctx->stream);
    delete ctx;
    return PTAM_OK;
}

int ptam_ctx_set_halfsample(ptam_ctx* ctx, int variant) {
    ARG_TRY(ctx && (variant == PTAM_HALFSAMPLE_R || variant == PTAM_HALFSAMPLE_T));
    ctx->halfsample = variant;
    return PTAM_OK;
}

int ptam_ctx_sync(ptam_ctx* ctx) {
    ARG_TRY(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    return PTAM_OK;
}

void* ptam_ctx_stream(ptam_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int ptam_ctx_camera_constants(ptam_ctx* ctx, double out[8]) {
    ARG_TRY(ctx && out);
    out[0] = ctx->cam.fx;
    out[1] = ctx->cam.fy;
    out[2] = ctx->cam.cx;
    out[3] = ctx->cam.cy;
    out[4] = ctx->cam.two_tan;
    out[5] = ctx->cam.w_inv;
    out[6] = ctx->cam.largest_radius;
    out[7] = ctx->cam.max_r;
    return PTAM_OK;
}

int ptam_ctx_cache_hazards(ptam_ctx* ctx, long long* out) {
    ARG_TRY(ctx && out);
    HIP_TRY(hipSetDevice(ctx->device));
    unsigned long long a = 0, b = 0;
    int rc = pose_hazards_read_pose(ctx->stream, &a);
    if (!rc) rc = pose_hazards_read_trackmap(ctx->stream, &b);
    if (rc) return rc;
    HIP_TRY(ptam_stream_wait(ctx->stream));
    *out = (long long)(a + b);
    return PTAM_OK;
}

int ptam_ctx_one_pixel_dist(ptam_ctx* ctx, double* out) {
    ARG_TRY(ctx && out);
    *out = ctx->cam.one_pixel_dist;
    return PTAM_OK;
}

int ptam_dev_alloc(ptam_ctx* ctx, size_t bytes, void** dptr) {
    ARG_TRY(ctx && dptr);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));
    return PTAM_OK;
}
int ptam_dev_free(ptam_ctx* ctx, void* dptr) {
    ARG_TRY(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    HIP_TRY(hipFree(dptr));
    return PTAM_OK;
}
int ptam_dev_upload(ptam_ctx* ctx, void* dptr, const void* host, size_t bytes) {
    ARG_TRY(ctx && dptr && host);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dptr, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    return PTAM_OK;
}
int ptam_dev_download(ptam_ctx* ctx, void* host, const void* dptr, size_t bytes) {
    ARG_TRY(ctx && dptr && host);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(host, dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    return PTAM_OK;
}

int ptam_project_points(ptam_ctx* ctx, int n, const double* world_xyz, const double pose[12],
                        ptam_projection* out) {
    ARG_TRY(ctx && n >= 0 && pose && (n == 0 || (world_xyz && out)));
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t wb = (size_t)n * 24, ob = (size_t)n * sizeof(ptam_projection);
    void* scratch;
    int rc = ctx_scratch(ctx, wb + 128 + ob, &scratch);
    if (rc) return rc;
    double* d_world = (double*)scratch;
    double* d_pose = (double*)((char*)scratch + wb);
    ptam_projection* d_out = (ptam_projection*)((char*)scratch + wb + 128);
    HIP_TRY(hipMemcpyAsync(d_world, world_xyz, wb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_pose, pose, 96, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(project_points_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->cam, n,
                       d_world, d_pose, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    return PTAM_OK;
}

int ptam_reproject_points(ptam_ctx* ctx, int n, const double* world_xyz, const double pose[12], ptam_projection* inout) {
    ARG_TRY(ctx && n >= 0 && pose && (n == 0 || (world_xyz && inout)));
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t wb = (size_t)n * 24, ob = (size_t)n * sizeof(ptam_projection);
    void* scratch;
    int rc = ctx_scratch(ctx, wb + 128 + ob, &scratch);
    if (rc) return rc;
    double* d_world = (double*)scratch;
    double* d_pose = (double*)((char*)scratch + wb);
    ptam_projection* d_io = (ptam_projection*)((char*)scratch + wb + 128);
    HIP_TRY(hipMemcpyAsync(d_world, world_xyz, wb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_pose, pose, 96, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_io, inout, ob, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(reproject_points_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->cam, n, d_world, d_pose, d_io);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(inout, d_io, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    return PTAM_OK;
}

}   // extern "C"
