// wait_mapped.h — the library's one wait for words a kernel writes into host-mapped memory behind its results.
#pragma once
#include <atomic>

#include "common.h"

// Wait until arrived() holds (ptam_stream_wait sleeps on an interrupt: up to milliseconds to wake up); every 100 000 looks ask the
// runtime whether the queue died instead.  A queue that has drained without the words gets 50 more polls, then it is a logic error,
// not a wait.  report(drained) is called at every 100th poll: a diagnostic of the caller's (the bundle prints its mailbox under
// PTAM_DEBUG_WAIT=1).  A wait that ends within 100 000 looks makes no HIP call.
template <class Arrived, class Report>
static int ptam_wait_mapped(hipStream_t stream, const char* what, Arrived arrived, Report report) {
    unsigned spins = 0, polls = 0, idle_polls = 0;
    while (!arrived()) {
        if (++spins < 100000) continue;
        spins = 0;
        const hipError_t q = hipStreamQuery(stream);
        if (q != hipSuccess && q != hipErrorNotReady) {
            ptam_set_error("the device queue failed while the host waited for %s: %s", what, hipGetErrorString(q));
            return PTAM_E_HIP;
        }
        if ((++polls % 100) == 0) report(q == hipSuccess);
        if (q == hipSuccess && !arrived() && ++idle_polls > 50) {
            ptam_set_error("the device queue drained and %s never arrived", what);
            return PTAM_E_STATE;
        }
    }
    if (polls) (void)hipGetLastError();   // (the runtime was asked: hipErrorNotReady is sticky in the last-error slot)
    std::atomic_thread_fence(std::memory_order_acquire);
    return PTAM_OK;
}
template <class Arrived>
static int ptam_wait_mapped(hipStream_t stream, const char* what, Arrived arrived) {
    return ptam_wait_mapped(stream, what, arrived, [](bool) {});
}
