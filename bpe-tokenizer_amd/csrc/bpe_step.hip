// bpe_step.hip — the table-state merge pass of the device loop (k_step_loop<MODE_TABLE>, the
// C3 hot path) in a translation unit of its own, compiled with
// -mllvm -structurizecfg-skip-uniform-regions (bpe-tokenizer_amd/Makefile).  With the flag the
// uniform branches of the ring stay scalar branches instead of lane-mask regions: k_step_loop
// 0.789 -> 0.775 ms at C3 (tools/ab_exp.sh, profiles/r03_ab_skip_uniform.json).  The same flag
// made the maintained-state pass (MODE_INCR) 2 % slower on zipf C3, so only this instantiation
// takes it, with its own scheduling flags and ring depth (Makefile STEP_FLAGS).
//
// The pass's header (bpe_pass.hip.h, the part of the kernels this unit launches from) is included
// with internal linkage (an anonymous namespace), so its kernels are not defined twice in
// libbpe.so; the launcher therefore takes the engine's structures as untyped pointers (same
// layout: the same header).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <type_traits>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"   // (the header's other instantiations)
namespace {
#include "bpe_pass.hip.h"
}
#pragma clang diagnostic pop

namespace bpe_step {

hipError_t launch_step_loop_table(unsigned grid, hipStream_t s, int32_t *ids, int64_t n_chunks,
                                  int64_t cpr, int R, const void *carry, const void *ctl,
                                  uint32_t *partials, unsigned long long *spill, const void *ct,
                                  void *sums, unsigned long long *replaced) {
    using namespace bpe;
    k_step_loop<MODE_TABLE><<<grid, WG, 0, s>>>(
        ids, n_chunks, cpr, R, static_cast<const RegionCarry *>(carry),
        static_cast<const LoopCtl *>(ctl), partials, spill, *static_cast<const ColdTable *>(ct),
        static_cast<RegionSum *>(sums), replaced);
    return hipGetLastError();
}

// The delta form's apply-only stream (k_apply_loop): the same ring, built with the same flags,
// and beside it the stream over the digest plane (digest_body; plane: one byte per slot, read
// only when the LoopCtl says it is fresh; lists, rows: the hit lists of the candidate pairs).
hipError_t launch_apply_loop(unsigned grid, hipStream_t s, int32_t *ids, int64_t n_chunks,
                             int64_t cpr, int R, const void *carry, void *ctl, void *sums,
                             unsigned long long *replaced, uint32_t *site_list, uint32_t *site_n,
                             uint32_t *plane, void *lists, uint32_t *rows) {
    using namespace bpe;
    // The scan's candidate-mask table is DG_TABLE bytes of dynamic LDS: beside the kernel's few
    // static bytes that is more than the 64 KiB a launch gets unasked, so the limit is raised
    // once per device.  One 1024-thread workgroup per CU is the shape already: the bytes cost no
    // occupancy, and the int32 body and a list iteration never touch them.
    static std::atomic<uint64_t> raised{0};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(raised.load(std::memory_order_relaxed) & bit)) {
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_apply_loop),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, DG_TABLE);
            e != hipSuccess)
            return e;
        raised.fetch_or(bit, std::memory_order_relaxed);
    }
    k_apply_loop<<<grid, WG, DG_TABLE, s>>>(ids, n_chunks, cpr, R, static_cast<const RegionCarry *>(carry),
                                     static_cast<LoopCtl *>(ctl), static_cast<RegionSum *>(sums),
                                     replaced, site_list, site_n, plane,
                                     static_cast<DigestLists *>(lists), rows);
    return hipGetLastError();
}

// The digest plane of the whole corpus (k_digest_build).
hipError_t launch_digest_build(hipStream_t s, const int32_t *ids, int64_t n_chunks, uint32_t *plane) {
    using namespace bpe;
    const int64_t blocks = (n_chunks * (CHUNK / 4) + 255) / 256;
    k_digest_build<<<(unsigned)(blocks < 1 ? 1 : blocks > 16384 ? 16384 : blocks), 256, 0, s>>>(
        ids, n_chunks, plane);
    return hipGetLastError();
}

// The host path's passes of the table state (findNextMerge / applyMerge one call each, the counts
// after a compaction, core.ts:247-360): k_step<NO_MERGE | MERGE_XY | MERGE_XX, MODE_TABLE>, built
// here with the same flags as the device loop's pass (in the engine's translation unit, with its
// 6-slot ring and default flags, the merge pass timed 0.80-0.82 ms at C3 against 0.74 here).
hipError_t launch_step_table(int merge, unsigned grid, hipStream_t s, int32_t *ids, int64_t n_chunks,
                             int64_t cpr, int R, const void *carry, int32_t ma, int32_t mb,
                             int32_t mc, uint32_t *partials, unsigned long long *spill,
                             const void *ct, const uint32_t *heavy, void *sums,
                             unsigned long long *replaced) {
    using namespace bpe;
    const RegionCarry *rc = static_cast<const RegionCarry *>(carry);
    const ColdTable &t = *static_cast<const ColdTable *>(ct);
    RegionSum *su = static_cast<RegionSum *>(sums);
    if (merge == MERGE_XX)
        k_step<MERGE_XX, MODE_TABLE><<<grid, WG, 0, s>>>(ids, n_chunks, cpr, R, rc, ma, mb, mc,
                                                        partials, spill, t, heavy, su, replaced);
    else if (merge == MERGE_XY)
        k_step<MERGE_XY, MODE_TABLE><<<grid, WG, 0, s>>>(ids, n_chunks, cpr, R, rc, ma, mb, mc,
                                                        partials, spill, t, heavy, su, replaced);
    else
        k_step<NO_MERGE, MODE_TABLE><<<grid, WG, 0, s>>>(ids, n_chunks, cpr, R, rc, ma, mb, mc,
                                                        partials, spill, t, heavy, su, replaced);
    return hipGetLastError();
}

}  // namespace bpe_step
