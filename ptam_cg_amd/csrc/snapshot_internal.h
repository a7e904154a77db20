// snapshot_internal.h — ptam_map_snapshot (ptam_hip.h): the map as the tracker wants it, published by ptam_rmap_publish
// (maprmap.hip) and taken by ptam_tracker_take_map (trackmap.hip).  Three slots of device memory; which one is whose is host
// state (snapshot_slots.h).  mapsnapshot.hip owns the memory.
#pragma once
#include "common.h"
#include "snapshot_slots.h"
#include "track_internal.h"   // TmSrc

struct SnapSlot {
    ptam_pvs_point* pts = nullptr;
    TmSrc* src = nullptr;
    long long* serials = nullptr;
    size_t cap = 0;              // points
    // what the slot holds: written by the publisher before its commit, read by a take after begin_read
    int n = 0;
    long long map_id = 0, generation = 0;
    // the keyframe section (ptam_snapshot_keyframes_enable; sbi.hip owns it): the poses and the SmallBlurryImages of keyframes
    // [0, kf_n) of map (kf_map_id, kf_epoch), in the layout of a ptam_sbi_bank.  The images outlive a generation: a publish of the
    // same map makes only the entries from kf_n on.  kf_generation == generation: the section belongs to what the slot holds.
    void* kf_block = nullptr;
    uint8_t* kf_small = nullptr;
    float* kf_tmpl = nullptr;
    float* kf_jacs = nullptr;
    double* kf_poses = nullptr;
    int kf_n = 0, kf_made = 0;   // kf_made: the entries the slot's last publish made
    long long kf_map_id = 0, kf_epoch = 0, kf_generation = 0;
};

struct ptam_map_snapshot {
    int device, width, height;   // of the context it was created from
    long long uid;               // process-wide: a tracker remembers (uid, generation) of its last take
    size_t want;                 // the capacity ptam_map_snapshot_reserve asked for
    SnapSlots slots;
    SnapSlot slot[SnapSlots::SLOTS];
    int kf_max = 0;              // 0: the keyframe section is not enabled
    double kf_blur = 0.0;
};

// slot s holds at least `rows` points (at least snap->want, or double what it held): the caller owns the slot — it is the
// publisher's, or idle.  What the slot held is gone.  *grew (nullable) is set when memory was allocated.
int snap_slot_room(ptam_map_snapshot* snap, int s, size_t rows, int* grew);
