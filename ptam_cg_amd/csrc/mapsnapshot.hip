// mapsnapshot.hip — ptam_map_snapshot (ptam_hip.h): the memory of the three slots.  The slot rules are snapshot_slots.h, the
// publish is ptam_rmap_publish (maprmap.hip), the take ptam_tracker_take_map (trackmap.hip).  No kernel lives here.
#include <algorithm>
#include <atomic>

#include "snapshot_internal.h"

static std::atomic<long long> g_snapshot_uid{0};

static void snap_slot_free(SnapSlot& sl) {
    if (sl.pts) (void)hipFree(sl.pts);
    if (sl.src) (void)hipFree(sl.src);
    if (sl.serials) (void)hipFree(sl.serials);
    sl.pts = nullptr;
    sl.src = nullptr;
    sl.serials = nullptr;
    sl.cap = 0;
}

int snap_slot_room(ptam_map_snapshot* snap, int s, size_t rows, int* grew) {
    SnapSlot& sl = snap->slot[s];
    if (rows <= sl.cap) return PTAM_OK;
    const size_t cap = std::max(std::max(rows, 2 * sl.cap), std::max(snap->want, (size_t)64));
    snap_slot_free(sl);
    if (hipMalloc((void**)&sl.pts, cap * sizeof(ptam_pvs_point)) != hipSuccess || hipMalloc((void**)&sl.src, cap * sizeof(TmSrc)) != hipSuccess ||
        hipMalloc((void**)&sl.serials, cap * sizeof(long long)) != hipSuccess) {
        snap_slot_free(sl);
        ptam_set_error("ptam_map_snapshot: no device memory for %zu points", cap);
        return PTAM_E_HIP;
    }
    sl.cap = cap;
    if (grew) *grew = 1;
    return PTAM_OK;
}

extern "C" {

int ptam_map_snapshot_create(ptam_ctx* ctx, int max_points, ptam_map_snapshot** out) {
    ARG_TRY(ctx && out && max_points >= 0);
    HIP_TRY(hipSetDevice(ctx->device));
    ptam_map_snapshot* s = new ptam_map_snapshot();
    s->device = ctx->device;
    s->width = ctx->params.width;
    s->height = ctx->params.height;
    s->uid = ++g_snapshot_uid;
    s->want = (size_t)max_points;
    for (int k = 0; k < SnapSlots::SLOTS; k++)
        if (int rc = snap_slot_room(s, k, std::max((size_t)max_points, (size_t)1), nullptr)) {
            ptam_map_snapshot_destroy(s);
            return rc;
        }
    *out = s;
    return PTAM_OK;
}

int ptam_map_snapshot_destroy(ptam_map_snapshot* s) {
    if (!s) return PTAM_OK;
    (void)hipSetDevice(s->device);
    for (int k = 0; k < SnapSlots::SLOTS; k++) {
        snap_slot_free(s->slot[k]);
        if (s->slot[k].kf_block) (void)hipFree(s->slot[k].kf_block);   // (the keyframe section, sbi.hip)
    }
    delete s;
    return PTAM_OK;
}

int ptam_map_snapshot_reserve(ptam_map_snapshot* s, int max_points) {
    ARG_TRY(s && max_points >= 0);
    HIP_TRY(hipSetDevice(s->device));
    s->want = std::max(s->want, (size_t)max_points);
    // (the mapmaker's thread: no publish is under way.  The current slot and one a take is copying keep what they hold and grow
    //  when they are next written.)
    for (int k = 0; k < SnapSlots::SLOTS; k++)
        if (s->slots.idle(k))
            if (int rc = snap_slot_room(s, k, s->want, nullptr)) return rc;
    return PTAM_OK;
}

int ptam_map_snapshot_info(ptam_map_snapshot* s, ptam_map_snapshot_info_t* out) {
    ARG_TRY(s && out);
    long long gen = 0;
    ptam_map_snapshot_info_t r = {};
    const int k = s->slots.begin_read(-1, &gen);   // (-1 is no generation: the current slot, held while it is read)
    if (k >= 0) {
        r.generation = s->slot[k].generation;
        r.map_id = s->slot[k].map_id;
        r.n_points = s->slot[k].n;
        s->slots.end_read(k);
    }
    *out = r;
    return PTAM_OK;
}

}   // extern "C"
