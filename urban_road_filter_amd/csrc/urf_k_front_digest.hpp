/*
 * urf_k_front_digest.hpp -- k_front_digest: the learning pass of urf_set_front_auto (include/urf.h) folds k_front_explain's per-scan
 * records into eight words the host reads without waiting (urf_policy::fold, urf_policy::auto_digest).
 *
 * One thread per scan evaluates urf_front_scan_rule (urf_k_front_explain.hpp: the rule urf_front_explain's host loop applies) on the
 * scan's record, its flag, its candidate count, its status and its length.  A wave reduces with ballots and one butterfly, and adds into
 * the pass's accumulator in device memory with one atomic per word that is not zero.  The block that draws the last ticket copies the
 * accumulator into the pass's host-mapped slot and, behind a system-scope fence, stores the sequence number the host handed to the pass:
 * a slot whose first word is not that number has not arrived.  Every store is a vector lane's.
 *
 * Grid ceil(n_scans / 256) blocks of 256 threads.  No LDS, no scratch memory.  Off the hot path: at most five calls per new start of a
 * context that turned the switch on launch it; a context that did not launches and allocates nothing.
 */
#ifndef URF_K_FRONT_DIGEST_HPP
#define URF_K_FRONT_DIGEST_HPP

#include "urf_k_front_explain.hpp"

/* the digest, in the order of urf_front_auto_info's digest_* fields */
#define URF_DG_SEQ 0u
#define URF_DG_SCANS 1u         /* scans with a result (URF_OK, not empty) */
#define URF_DG_HANDED_BACK 2u   /* ... of those, the ones whose flag is cleared */
#define URF_DG_SCAN_BITS 3u     /* OR of the URF_WHY_SCAN_* bits of the handed-back scans */
#define URF_DG_HELPED 4u        /* handed-back scans whose bits are MULTI_SECTOR / SECTORS_FALL and nothing else */
#define URF_DG_NEVER 5u         /* ... with one of the four shape bits or ROWS_LENGTH */
#define URF_DG_CANDIDATES 6u
#define URF_DG_OTHER 7u
#define URF_DG_WORDS 8u
/* the accumulator: the digest's words (word 0: the ticket counter instead of the sequence number), zeroed by the host in front of the pass */
#define URF_DG_SCAN_NEVER (URF_WHY_SCAN_LANE_TWO_RINGS | URF_WHY_SCAN_RING_TWO_LANES | URF_WHY_SCAN_AXIS | URF_WHY_SCAN_RANGE | URF_WHY_SCAN_ROWS_LENGTH)
#define URF_DG_SCAN_HELPED (URF_WHY_SCAN_MULTI_SECTOR | URF_WHY_SCAN_SECTORS_FALL)

__global__ __launch_bounds__(256) void k_front_digest(urf_kargs a, urf_fx_call call, const uint32_t* __restrict__ recs, uint32_t* acc, uint32_t* slot,
                                                      uint32_t seq)
{
    const unsigned s = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool counted = false;
    uint32_t scan = 0u;
    if (s < a.n_scans) {
        unsigned off, len;
        urf_scan_range(a, s, off, len);
        if (call.len != 0u && len != 0u)
            len = call.len;   /* (a sweep that runs padded: the caller's points) */
        const int status = a.info[s].status;
        const urf_fx_scan v = urf_front_scan_rule(call, recs + (size_t)s * URF_FX_WORDS, a.front_ok[s], a.front_ncand[s], status, len);
        counted = status == URF_OK && len != 0u;
        if (counted && !v.fused)
            scan = v.scan | 0x80000000u;   /* (handed back, whatever its bits) */
    }
    const bool back = scan != 0u;
    const unsigned n_scans = (unsigned)__popcll(__ballot(counted));
    const unsigned n_back = (unsigned)__popcll(__ballot(back));
    const unsigned n_helped = (unsigned)__popcll(__ballot(back && (scan & 0x7fffffffu & ~URF_DG_SCAN_HELPED) == 0u && (scan & URF_DG_SCAN_HELPED) != 0u));
    const unsigned n_never = (unsigned)__popcll(__ballot(back && (scan & URF_DG_SCAN_NEVER) != 0u));
    const unsigned n_cand = (unsigned)__popcll(__ballot(back && (scan & URF_WHY_SCAN_CANDIDATES) != 0u));
    const unsigned n_other = (unsigned)__popcll(__ballot(back && (scan & URF_WHY_SCAN_OTHER) != 0u));
    uint32_t bits = scan & 0x7fffffffu;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        bits |= (uint32_t)__shfl_xor((int)bits, d);
    if (lane == 0u) {
        if (n_scans)
            atomicAdd(&acc[URF_DG_SCANS], n_scans);
        if (n_back)
            atomicAdd(&acc[URF_DG_HANDED_BACK], n_back);
        if (bits)
            atomicOr(&acc[URF_DG_SCAN_BITS], bits);
        if (n_helped)
            atomicAdd(&acc[URF_DG_HELPED], n_helped);
        if (n_never)
            atomicAdd(&acc[URF_DG_NEVER], n_never);
        if (n_cand)
            atomicAdd(&acc[URF_DG_CANDIDATES], n_cand);
        if (n_other)
            atomicAdd(&acc[URF_DG_OTHER], n_other);
        __threadfence();   /* this wave's adds, in front of the block's ticket */
    }
    __syncthreads();
    if (threadIdx.x != 0u)
        return;
    if (atomicAdd(&acc[0], 1u) != gridDim.x - 1u)
        return;
    __threadfence();   /* the last block: every other block's adds came in front of its ticket */
    for (unsigned w = 1u; w < URF_DG_WORDS; w++)
        __hip_atomic_store(&slot[w], __hip_atomic_load(&acc[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __hip_atomic_store(&slot[URF_DG_SEQ], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

#endif /* URF_K_FRONT_DIGEST_HPP */
