// framereport_internal.h — ptam_frame_report (ptam_hip.h) as the three files that touch it see it: the object (framereport.hip), the
// tracker's front (trackmap.hip: ptam_tracker_report_frames) and the resident map's consumers (maprmap.hip).  Front / core as in
// maptables_internal.h: a front says where one frame's iteration set lies (FrJob, every pointer a device pointer) and uploads the
// job table; the core fr_fill_core only enqueues.
#pragma once
#include "map_stage.h"

struct ptam_frame_report {
    ptam_ctx* ctx;
    int max_records;
    ptam_frame_record* rec;     // device: max_records records, the first info.n_records valid
    int* mark;                  // device work: one word per point of the frame's map, grown on demand
    size_t mark_cap;
    ptam_frame_report_info_t info;
};

// One frame's iteration set, as the host supplied it (entries != null) or where the tracker left it (the columns of TmDev; the
// set's length, the measurement count and the outlier layout are read from the tracker's control block on the device: nothing
// comes down before the fill).
struct FrJob {
    int n_points;                           // the map the set's point indices count in
    const long long* serials;               // [n_points], strictly increasing
    const ptam_trackmap_meas* entries;      // host-supplied rows, or null
    int n_entries;                          //   their count
    int cap;                                // tracker: the columns' capacity (the set's length is clamped to it)
    const int *n_slots, *n_meas, *outlier_by_slot;   // tracker: TmCtl's words
    const int *list, *slot_found, *slot_subpix;
    const ptam_patch_query* q;
    const ptam_template_result* tres;
    const double2* slot_v2;
    const int *outlier, *mslot;             // outlier: at the slots (outlier_by_slot) or at the measurements, mslot[k] = measurement k's slot (ascending)
    int* mark;                              // work: n_points words
    ptam_frame_record* rec;                 // out: room for max_records
    int max_records;
};
static_assert(sizeof(FrJob) == 144, "what ptam_hip.h says a fill sends up per camera");
enum { FR_H_RECORDS = 0, FR_H_OUTLIERS, FR_H_ENTRIES, FR_H_PAD, FR_HEAD_WORDS };   // what a fill leaves per job: 16 bytes
// d_jobs: nb jobs in device memory; d_heads: nb x FR_HEAD_WORDS.  One launch, one workgroup per job.  FR_H_RECORDS is the found
// points' count even where it exceeds max_records (nothing is written behind max_records).
int fr_fill_core(hipStream_t st, int nb, const FrJob* d_jobs, int* d_heads);
// A job of the fill that closes a batch chain: the heads go to host-mapped words, the sequence number behind them.
struct FrChainJob {
    FrJob job;
    const int* gate;                          // nullable: *gate == 0 — the frame tracked nothing, the head is zero, job is not looked at
    const unsigned long long* frame_word;     // the frame's published sequence word: FR_FRAME_LONG in it — not finished, nothing is done
    int* head;                                // FR_HEAD_WORDS words, host-mapped
    unsigned long long* head_seq;             // host-mapped: = seq once head and the records are written
    unsigned long long seq;
};
static_assert(sizeof(FrChainJob) == 184, "what ptam_hip.h says the chain's fill sends up per report");
#define FR_FRAME_LONG (1ull << 63)   // POSE_CHAIN_LONG (track_internal.h)
int fr_fill_chain_core(hipStream_t st, int nb, const FrChainJob* d_jobs);
// the report's mark array holds n_points words (the one allocation a fill may make)
int fr_mark_room(ptam_frame_report* r, int n_points);
