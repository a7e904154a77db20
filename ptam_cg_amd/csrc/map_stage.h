// map_stage.h — the carve of one allocation (Carver) and the staging of one map call on one context (MapStage): the call's one
// request to the context's scratch with the pinned request beside it, the copies up and down, the byte counters they feed.
#pragma once
#include "common.h"

// carves one allocation into 256-byte aligned pieces: take() returns the piece's offset, `off` ends as the size of the whole.
// piece<T>(count) returns the piece itself, so that a layout names each piece once: it is a function of a Carver that is run twice,
// first without a base for the size of the whole (the pointers it hands out then mean nothing), then with the block's address.
// room<T>(count) is a piece that keeps a byte when count is 0: for what a memset or a kernel argument is derived from.
struct Carver {
    char* base = nullptr;
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
    template <class T>
    T* piece(size_t count) { return (T*)((uintptr_t)base + take(count * sizeof(T))); }
    template <class T>
    T* room(size_t count) { return (T*)((uintptr_t)base + take(count > 0 ? count * sizeof(T) : 1)); }
};

// One map call's staging.  carve(layout) runs `layout(Carver& dev, Carver& pin)` twice, for the sizes and with the two blocks, and
// between the runs asks the context ONCE for each: ctx_scratch hands out one block per context, so whatever a call carves from it
// has to come from one request (a second, larger one would free the block under the first one's queued work).  A pinned piece's
// device address is pin_dev(p).  up / down skip zero bytes and add to the counters (the resident map's traffic, or nobody's).
struct MapStage {
    ptam_ctx* ctx;
    hipStream_t st;
    unsigned long long *h2d, *d2h;   // nullable
    explicit MapStage(ptam_ctx* c, unsigned long long* up_bytes = nullptr, unsigned long long* down_bytes = nullptr)
        : ctx(c), st(c->stream), h2d(up_bytes), d2h(down_bytes) {}

    template <class Layout>
    int carve(Layout&& layout) {
        Carver dev_size, pin_size;
        layout(dev_size, pin_size);
        void *sc = nullptr, *hp = nullptr;
        if (dev_size.off > 0)
            if (int rc = ctx_scratch(ctx, dev_size.off, &sc)) return rc;
        if (pin_size.off > 0)
            if (int rc = ctx_pinned(ctx, pin_size.off, &hp)) return rc;
        Carver dev{(char*)sc}, pin{(char*)hp};
        layout(dev, pin);
        return PTAM_OK;
    }
    template <class T>
    T* pin_dev(T* pinned_piece) const { return (T*)((char*)ctx->d_pinned + ((char*)pinned_piece - (char*)ctx->h_pinned)); }

    int up(void* dst, const void* src, size_t bytes) {
        if (bytes == 0) return PTAM_OK;
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        if (h2d) *h2d += bytes;
        return PTAM_OK;
    }
    int down(void* dst, const void* src, size_t bytes) {
        if (bytes == 0) return PTAM_OK;
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        if (d2h) *d2h += bytes;
        return PTAM_OK;
    }
    static unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }
};
#define STAGE_TRY(expr)                 \
    do {                                \
        if (int rc__ = (expr)) return rc__; \
    } while (0)

// ptam_map_scene_depth behind its upload (mapalign.hip): tables in device memory, n_kf > 0, h_out in the stage's pinned block, out on
// the host; one launch, one wait
int map_scene_depth_core(MapStage& s, int n_kf, const double* d_poses, const double* d_points3, int n_meas, const ptam_map_meas* d_meas,
                         ptam_scene_depth* h_out, ptam_scene_depth* out);
// ptam_map_apply_global_transform's launch on device tables (mapalign.hip), its 256-byte record in the caller's stage: enqueues only
int map_transform_core(MapStage& s, void* d_record, void* h_record, const double se3_new_from_old[12], int K, const double* d_poses,
                       double* d_poses_new, int N, double* d_points3, const ptam_map_point_source* d_src, ptam_pvs_point* d_pvs, int pvs_stride);
// ... and the launch alone, on an aligner's record that is in device memory already (the plane stage's, or one uploaded): K + N > 0
int map_apply_core(MapStage& s, const void* d_record, int K, const double* d_poses, double* d_poses_new, int N, double* d_points3,
                   const ptam_map_point_source* d_src, ptam_pvs_point* d_pvs, int pvs_stride);
// CalcPlaneAligner (mapalign.hip) on a point table in device memory.  The pieces of the caller's stage (map_plane_layout), then
// map_plane_core: the draw (or the caller's samples) up, plane_score_kernel and plane_finish_kernel; enqueues only.  The aligner's
// 256-byte record is left at w.d_record for map_apply_core and arrives, through host-mapped memory, at w.h_record: after the
// caller's wait map_plane_result reads the info and the aligner there.  Options checked by the caller (map_plane_check).
struct MapPlaneWork {
    int32_t *d_samples, *h_samples;
    double* scores;
    int* skipped;
    char* d_record;   // 256 bytes, then the n inlier bytes
    char* h_record;   // pinned, 256 bytes
};
int map_plane_check(int n, const ptam_plane_opts* o);   // PTAM_E_ARG as ptam_calc_plane_aligner refuses its options
void map_plane_layout(Carver& c, Carver& pin, int n, int trials, MapPlaneWork& w);
int map_plane_core(MapStage& s, const MapPlaneWork& w, const ptam_plane_opts* o, int n, const double* d_points3);
void map_plane_result(const MapPlaneWork& w, ptam_plane_info* info, double se3_aligner[12]);
// the record of a caller's own aligner (status PTAM_PLANE_OK), or of no move at all (status PTAM_PLANE_TOO_FEW: map_apply_core then
// copies the poses, leaves the points and refreshes the pixel vectors alone), into 256 pinned bytes and up to d_record
int map_record_up(MapStage& s, void* d_record, void* h_record, int status, const double se3_new_from_old[12]);
