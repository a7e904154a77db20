// refind_internal.h — the pair-list finder chain of refind.hip (ReFind_Common through ONE PatchFinder), for the callers that write
// its pair records on the device (maprefind.hip).
#pragma once
#include "track_internal.h"

struct RpPair {
    ptam_pvs_point pt;
    TmSrc src;
    double pose[12];
    long long id;
    int skip, kf;
};
struct RpFinder {   // the state of the reference's static PatchFinder that outlives a call
    long long pt;          // mpLastTemplateMapPoint
    double m2[4];          // mm2LastWarpMatrix {m00, m01, m10, m11}
    int valid, bad;        // mpLastTemplateMapPoint != NULL, mbTemplateBad
    uint8_t tpl[64];       // mimTemplate
};
struct RpDev {
    int n;
    const RpPair* pairs;
    const KfLevels* Ls;
    TemplateJob* jobs;
    ptam_patch_query* q;
    double* m2;            // [n][4]
    int* reach;            // the pair gets as far as the finder
    int* detbad;           // CalcSearchLevelAndWarpMatrix rejects the warp
    int* R;                // reaching pairs, in order
    int* nr;
    int* refresh;          // the finder re-makes its template for this pair
    int* srcp;             // pair whose template this pair searches with (-1: the template the finder brought along)
    int* dacc;             // a warp was rejected since that template was made (this pair's included)
    int* bad;              // Finder.TemplateBad() for this pair
    uint8_t* tm;           // [n][64]
    ptam_template_result* tres;
    RpFinder* st;
    ptam_refind_result* out;
    int* kept;
};
struct ptam_refinder {
    ptam_ctx* ctx;
    RpFinder* st;   // device
};
// the chain's work arrays for n pairs, carved out of b from `off` on (everything of RpDev but n, pairs, Ls and st) -> the offset
// behind them; b == nullptr only measures
size_t rp_carve(RpDev& d, char* b, size_t off, int n);
// the five launches of the chain on d.n pairs (d.n > 0), enqueued on st
void rp_launch_chain(hipStream_t st, const DevCam& cam, const RpDev& d);
