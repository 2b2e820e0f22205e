// fbsmi_host.h -- host-side helpers shared by the translation units of libfbsmi.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace fbsmi {

// caller-provided scratch, carved by carve(): see fbsmi_workspace_bytes()
struct Workspace {
    float* part0;  // per-workgroup partial sums
    float* part1;  // per-workgroup partial maxima
    float* pref;   // top-level (P, E) per partial (only when the partials exceed one in-kernel tree)
    float* pend;
    float* scal;   // 64 scalars
    float* tmp0;   // n+1 floats
    float* tmp1;
    float* tmp2;
};

int fail(int code, const std::string& msg);
Workspace carve(void* ws, int64_t n);
int items_for(int64_t n);

#define FBSMI_HIP_TRY(call)                                                                         \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) return ::fbsmi::fail(-2, std::string(#call ": ") + hipGetErrorString(e_)); \
    } while (0)

// Run `enqueue` on st: directly, or (use_graph) as a graph captured on first use into `slot` and replayed from then on.
template <typename Enqueue>
int launch_captured(hipGraphExec_t& slot, hipStream_t st, bool use_graph, Enqueue&& enqueue) {
    if (!use_graph) return enqueue();
    if (!slot) {
        hipGraph_t g = nullptr;
        FBSMI_HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
        int rc = enqueue();
        hipError_t e = hipStreamEndCapture(st, &g);
        if (!rc && e != hipSuccess) rc = fail(-2, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        if (!rc && (e = hipGraphInstantiate(&slot, g, nullptr, nullptr, 0)) != hipSuccess)
            rc = fail(-2, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        if (g) (void)hipGraphDestroy(g);
        if (rc) return rc;
    }
    FBSMI_HIP_TRY(hipGraphLaunch(slot, st));
    return 0;
}

}  // namespace fbsmi
