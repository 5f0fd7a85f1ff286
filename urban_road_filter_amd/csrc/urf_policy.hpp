/* urf_policy.hpp -- the launch policy of the host API: which kernels a call launches (urf_policy::plan) and which family of the fused
 * front end they belong to (urf_front_family_of); the callback path's urf_sweep_shape and urf_seq_cache.  Host code without a HIP call:
 * it compiles with a plain C++17 compiler, and tests/cpp/policy_*.cpp walk its decisions without a GPU. */
#ifndef URF_POLICY_HPP
#define URF_POLICY_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "urf_internal.hpp"

struct urf_ctx;
struct ihipStream_t;   /* (hipStream_t is a pointer to it: fold() is the one member that needs HIP, defined in urf_api.hip) */

/* ---- what only the host's decision reads of the fused front end (the kernels: urf_front.hpp) ---- */
#define URF_FRONT_MIN_SCANS 192u  /* below (mode 1): the general kernels.  A block of k_front is ONE wave marching 80-144 dependent steps, k_front_finish one
                                   * workgroup per scan: with few scans the device is empty and the chains are the time (tools/r6_min_scans.py, general / fused ms per call:
                                   * 32 sweeps 0.21 / 0.25-0.33, 64: 0.31 / 0.32-0.40, 128: 0.45 / 0.44-0.50, 256: 0.73 / 0.66-0.70, 1024: 2.44 / 2.1) */
#define URF_FRONT_MIN_SCANS_32 0xffffffffu   /* 32 / 16 lasers per firing, mode 1: never (mode 2 only) */
#define URF_FRONT_MIN_SCANS_16 0xffffffffu
#define URF_FRONT_TPB_SMALL 2u    /* tiles per block of k_front for batches below URF_FRONT_TPB_SCANS scans (more, shorter chains), ... */
#define URF_FRONT_TPB_LARGE 4u    /* ... and from there on (less halo): 256 sweeps 0.663 / 0.703 ms at 2 / 4, 1024 sweeps 0.829 / 0.820 */
#define URF_FRONT_TPB_SCANS 512u
#define URF_FRONT_CP_MASK 0x1feu   /* curbPoints with a fused instance at 64 lasers (bit cp; 5 in every mode, the others with urf_set_front_mode(3)) */
/* ... and the values besides 5, for everything that exists once per value: the march at four laser counts (k_front*_cp<n>), the finish
 * kernels (k_front_finish*_cp<n>) and the host's choice among them (urf_front_family_of, urf_api.hip: front_kernels) */
#define URF_FRONT_CP_OTHERS(X) X(1) X(2) X(3) X(4) X(6) X(7) X(8)
#define URF_FRONT_MAX_TILES 128u  /* k_front_finish keeps a presence word per (tile, lane) in LDS */
#define URF_FRONT128_TILES2(tiles) (((tiles) + 1u) & ~1u)   /* a presence word covers 32 firings, two tiles of 128 lasers: words and block maxima are counted for an even number */
/* Entries per scan of the candidate lists of these kernels.  The points that pass the march's height tests are counted per LASER, not per
 * column: a ring that crosses a curb hands on up to eleven centres (z_zero) and six marked points (x_zero) per crossing, a street has four
 * crossings per ring -- 128 x 68 = 8 704 for 128 lasers however short the sweep is (a 128 x 256 street of urf_synth_cloud: 5 200 - 5 600),
 * above the context's max(max_points / 8, 4096) for sweeps below 128 x 544.  Twice that for range noise; a list that overflows still only
 * hands its scan back.
 * curbPoints 1..8 (urf_set_front_curb_points): 2 * CP + 1 centres and CP + 1 marked points per crossing, at 8 that is 17 and 9 -- 4 x 26 = 104 per
 * laser: 128 x 104 = 13 312 here, below the cap as it is; 32 x 104 = 3 328 and 16 x 104 = 1 664 at 32 and 16 lasers, below the context's floor of
 * 4096 (a block's border adds at most 2 * CP edge items per laser: 16 more per block).  No cap grows for the new instances. */
#define URF_FRONT128_CAND_CAP(max_points) ((max_points) / 8u > 16384u ? (max_points) / 8u : 16384u)
/* Scans of 129..256 tiles (urf_set_front_long_sweeps; 256 tiles: a 128 x 4096 sweep): the same finish kernels with the dynamic LDS their
 * layout needs for that many tiles -- a presence word and a 16-bit count per (tile, lane), 384 B per tile, and the chunk of the candidate
 * list: 108 KiB at 256 tiles, one workgroup per CU instead of four.  A call of at most URF_FRONT_MAX_TILES tiles asks for what it always
 * asked for.  Nothing else in the fused kernels counts tiles: the 16-bit counts hold a lane's ring points in the tiles before, at most
 * 255 x 2048 / 16 < 65536 (16 lasers per firing). */
#define URF_FRONT_LONG_MAX_TILES 256u

/* urf_set_front_auto (urf_policy::auto_call / auto_digest): how often a digest may say "call again" per new start -- the suite's own
 * figure: its tests run three calls before they demand that every hand-back is explained --, and the advice auto never applies */
#define URF_AUTO_AGAIN_MAX 3u
#define URF_ADVICE_LEFT_MASK (URF_ADVICE_NEVER | URF_ADVICE_CAPACITY | URF_ADVICE_BATCH | URF_ADVICE_CAPTURE_OFF | URF_ADVICE_RESET | URF_ADVICE_FRONT_OUTPUTS | URF_ADVICE_CALL_AGAIN)

/* The launch policy: which kernels a call launches, decided on the host from what the kernels of earlier calls reported through the
 * host-mapped flag words (enum urf_flag).  fold() is the only reader of the words: a batch call runs it in run_pipeline, a sweep of the
 * callback path in urf_classify_pc2_async, before either launches anything.  plan() turns the fields into a call's urf_kargs.  Every
 * change of what plan() reads bumps `epoch` (set()), the key of the callback path's captured sequences: a replayed sequence launches
 * what a fresh one would.  (Hidden: the library exports the C ABI, not this struct's functions.) */
struct __attribute__((visibility("hidden"))) urf_policy {
    uint32_t* flags = nullptr;      /* [URF_FLAG_WORDS] pinned, device-mapped (urf_kargs::flags) */
    uint64_t epoch = 1;             /* bumped by everything a captured sequence depends on (the settings' entry points bump it too) */
    /* k_ring_table speculates: it stops when no new ring has shown up for a while (speculate) and at the ring count of the row's previous
     * call (use_hint).  k_split checks; a scan that proves a rule wrong is repaired in the same call and raises its flag word
     * (URF_FLAG_LOOKAHEAD_FAILED / URF_FLAG_HINT_FAILED), and the context does without that rule from then on. */
    bool speculate = true, use_hint = true;
    /* the callback path's short sequence leaves out what normally finds nothing to do; a sweep that needed the kernels for the work lists
     * of oversized star sectors (slot_lists), for rings with a point on the sensor's axis (slot_nan) or for equal planar ranges in a star
     * sector (slot_ties: any real sensor's sweep) comes back with a URF_STATUS_REDO_* status and is run again with them, as are all later
     * ones (on_redo) */
    bool slot_lists = false, slot_nan = false, slot_ties = false;
    /* the fused front end (urf_front.hpp, urf_set_front_mode): 0 never, 1 batches of at least URF_FRONT_MIN_SCANS scans (default), 2 every
     * batch call it applies to, 3 as 2 and curbPoints 1..8 at 64 lasers (every_batch(): 2 or 3).  After a read-back of ring-sorted results the
     * context keeps to the general kernels (want_ring_sorted, last_call). */
    int front_mode = 1;
    bool every_batch() const { return front_mode >= 2; }
    /* urf_set_front_lasers128: modes 2 and 3 take sweeps of 128 lasers per firing too (k_front128*, urf_front.hpp; its scratch is there) */
    bool lasers128 = false;
    /* urf_set_front_curb_points: mode 3 takes curbPoints 1..8 at 16, 32 and (lasers128) 128 lasers per firing too (k_front32_cp*,
     * k_front16_cp*, k_front128_cp*) */
    bool curb_points = false;
    /* urf_set_front_multi_sector: with the star-shaped search on and curbPoints 5 the march is a k_front*_ms instance and k_front_sectors
     * follows it (urf_k_front_sectors.hpp): firings that span several sectors, sectors that fall inside a tile stay fused.  Other
     * curbPoints: the plain instances ... */
    bool multi_sector = false;
    /* ... unless urf_set_front_multi_sector_curb_points is on as well: then whatever curbPoints the call's fused kernels have an instance
     * for (curb_points_ok: 1..8) has a multi-sector one (k_front*_ms_cp<n>).  Without multi_sector it decides nothing. */
    bool multi_sector_cp = false;
    bool long_sweeps = false;       /* urf_set_front_long_sweeps: modes 2 and 3 take scans of up to URF_FRONT_LONG_MAX_TILES tiles */
    uint32_t front_tpb = 0;         /* tiles per block of k_front; 0: by batch size (URF_FRONT_TPB_*), else what URF_FRONT_TPB says */
    bool want_ring_sorted = false;
    /* urf_set_front_outputs: the published order and the marker points of a fused call come from what it left on the device
     * (urf_k_front_outputs.hpp) instead of a second run through the general kernels.  Decides no launch of a classify call: not part of
     * the epoch. */
    bool front_outputs = false;
    /* urf_set_sweep_outputs (URF_SWEEP_OUT_*): a sweep's captured sequence also produces its marker points and / or ordered lists.  Part
     * of the epoch -- the slots capture again -- but not read by plan(): it decides no launch of the classification. */
    uint32_t sweep_outputs = 0;
    /* urf_set_sweep_results_direct: the kernels of such a sequence store those products themselves into mapped pinned memory of the sweep's
     * slot, the lists packed back to back, and the sequence holds no copy for them.  Part of the epoch, not read by plan(), as sweep_outputs. */
    bool sweep_direct = false;
    /* urf_set_sweep_quantum: a sweep of the callback path runs as the next multiple of this many points, NaN behind its own, and a slot
     * keeps a few captured sequences, one per padded length (0: off).  Part of the epoch, not read by plan(), as sweep_outputs. */
    uint32_t sweep_quantum = 0;
    /* k_front hands a scan without the shape back to the general kernels: launched list-driven until a call has done so
     * (URF_FLAG_FRONT_HANDED_BACK: front_direct, full grids from then on); mode 1 stops trying once a whole batch has been handed back
     * (URF_FLAG_FRONT_ALL_HANDED_BACK: front_off, unorganised clouds).  forget_front() starts over. */
    bool front_direct = false, front_off = false;
    /* row-major organised sweeps (k_ring_table's third rule): once one has been sighted (URF_FLAG_ROWS_SIGHTED) the firing-order copies are
     * allocated and the sequences hold k_rows_probe and k_transpose (front_rows; rows_oom: the allocation failed).  Once a scan has taken
     * the layout (URF_FLAG_ROWS_TAKEN: rows_used), or while the sighting is on probation, batches below mode 1's threshold and the
     * callback path take the fused kernels too. */
    bool front_rows = false, rows_oom = false, rows_used = false;
    uint32_t rows_probation = 0;

    /* urf_set_front_auto: the context applies urf_front_explain's advice itself, in modes 2 and 3 (every_batch()).  plan() reads none of
     * these fields; what auto applies goes through the setters' own code and reaches plan() as their fields.  auto_phase: URF_AUTO_*;
     * auto_applied / auto_refused: URF_ADVICE_* bits it turned on / could not have (URF_ERR_OOM); auto_again: CALL_AGAIN digests taken
     * since the last new start (at most URF_AUTO_AGAIN_MAX); auto_left / auto_left_digest: the advice of the last call / digest it never applies;
     * auto_explained: calls that carried the learning pass since the last new start.  auto_wait: 1 + the digest slot of the one pass in
     * flight (0: none), auto_seq: the sequence number handed to it -- fold() takes the digest once its first word is that number. */
    bool auto_on = false;
    uint32_t auto_phase = URF_AUTO_IDLE, auto_applied = 0, auto_refused = 0, auto_again = 0, auto_left = 0, auto_left_digest = 0, auto_explained = 0;
    uint32_t auto_wait = 0, auto_seq = 0;
    uint32_t auto_digest_words[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };   /* the digest fold() took last (urf_front_auto_query) */
    /* A new start of the learning: urf_set_params with other parameters, urf_set_front_mode with another mode (or ending a sticky
     * read-out), a switch setter that changes its switch, the row-major sighting, urf_set_front_auto(ctx, 1) -- whatever runs
     * forget_front() for a reason other than auto's own application.  A pass still in flight teaches nothing any more. */
    void auto_start()
    {
        if (!auto_on)
            return;
        auto_phase = every_batch() ? URF_AUTO_LEARNING : URF_AUTO_IDLE;
        auto_refused = auto_again = auto_explained = auto_wait = auto_left_digest = 0;
        for (uint32_t& w : auto_digest_words)   /* (the digest of other parameters or settings says nothing any more) */
            w = 0;
    }
    /* The URF_ADVICE_* bits to apply at a call, on the host, before it is planned: why() of the call under the settings as they are.
     * NEVER, CAPTURE_OFF and RESET name something auto does not touch, and with one of them missing no switch makes the call fused;
     * BATCH does not block (a sweep of the callback path may still be sighted row-major). */
    uint32_t auto_call(uint32_t why_bits, uint32_t advice) const
    {
        if (!auto_on || !every_batch() || !why_bits || (advice & (URF_ADVICE_NEVER | URF_ADVICE_CAPTURE_OFF | URF_ADVICE_RESET)))
            return 0u;
        return advice & URF_ADVICE_AUTO_MASK & ~auto_refused;
    }
    /* What a digest (k_front_digest: seq, scans, handed_back, scan_bits, helped, never, candidates, other) teaches: the bits to apply and
     * the next phase; again: the digest was one of the URF_AUTO_AGAIN_MAX that may say "call again". */
    struct auto_step { uint32_t apply, phase; bool again; };
    auto_step auto_digest(const uint32_t* d, const urf_dev_params& dp) const
    {
        if (!auto_on || !every_batch())
            return auto_step{ 0u, URF_AUTO_IDLE, false };
        if (d[4] > 0u) {   /* helped: the multi-sector march keeps those scans */
            const uint32_t want = URF_ADVICE_MULTI_SECTOR | (dp.p.curbPoints != 5 ? URF_ADVICE_MULTI_SECTOR_CP : 0u);
            const uint32_t have = (multi_sector ? URF_ADVICE_MULTI_SECTOR : 0u) | (multi_sector_cp ? URF_ADVICE_MULTI_SECTOR_CP : 0u);
            const uint32_t apply = want & ~have & ~auto_refused;
            if (apply)
                return auto_step{ apply, URF_AUTO_LEARNING, false };
        }
        if (d[2] == 0u || d[5] + d[6] == d[2])   /* nothing handed back, or nothing auto can lift */
            return auto_step{ 0u, URF_AUTO_SETTLED, false };
        if ((d[7] > 0u || (d[3] & URF_WHY_SCAN_ROWS_SIGHTING)) && auto_again < URF_AUTO_AGAIN_MAX)   /* a repaired speculation, a first sighting */
            return auto_step{ 0u, URF_AUTO_LEARNING, true };
        return auto_step{ 0u, URF_AUTO_SETTLED, false };
    }
    /* the advice in a digest that auto never applies (auto_left) */
    static uint32_t auto_digest_left(const uint32_t* d)
    {
        return (d[5] ? URF_ADVICE_NEVER : 0u) | (d[6] ? URF_ADVICE_CAPACITY : 0u) | ((d[7] || (d[3] & URF_WHY_SCAN_ROWS_SIGHTING)) ? URF_ADVICE_CALL_AGAIN : 0u);
    }

    template <class T>
    void set(T& field, T value)
    {
        if (field != value) {
            field = value;
            epoch++;
        }
    }
    /* urf_set_params with other parameters, urf_set_front_mode with another mode, the row-major sighting */
    void forget_front()
    {
        set(front_direct, false);
        set(front_off, false);
        flags[URF_FLAG_FRONT_HANDED_BACK] = flags[URF_FLAG_FRONT_ALL_HANDED_BACK] = 0;
    }
    int fold(urf_ctx* c, ihipStream_t* st);
    /* A sighting that no scan confirms (a sweep in firing order whose region of interest begins with a single laser) lapses after 16 calls
     * that count: every submission on the callback path, whichever kernels it takes, but only those batch calls below mode 1's threshold
     * that took the fused kernels on its strength. */
    void probation_sweep() { lapse(front_rows); }
    void probation_batch(const urf_kargs& a) { lapse(a.front && !every_batch() && a.n_scans < URF_FRONT_MIN_SCANS); }
    void lapse(bool counts)
    {
        if (counts && !rows_used && rows_probation && --rows_probation == 0)
            epoch++;
    }
    /* a sweep of the callback path that the short sequence voided: from now on the sequence holds what it needed (false: no such status) */
    bool on_redo(int status)
    {
        switch (status) {
        case URF_STATUS_REDO_TABLE: set(speculate, false); return true;
        case URF_STATUS_REDO_HINT: set(use_hint, false); return true;
        case URF_STATUS_REDO_LISTS: set(slot_lists, true); return true;
        case URF_STATUS_REDO_NAN: set(slot_nan, true); return true;
        case URF_STATUS_REDO_TIES: set(slot_ties, true); return true;
        }
        return false;
    }
    /* ---- what plan() asks of the settings, each question in one place ---- */
    /* the lasers per firing the fused kernels take: 64, 32 and 16; 128 with urf_set_front_lasers128 in modes 2 and 3 */
    bool lasers_ok(unsigned L) const { return L == 64u || L == 32u || L == 16u || (L == 128u && lasers128 && every_batch()); }
    /* the curbPoints they have an instance for: 5 in every mode; with urf_set_front_mode(3) and 64 lasers per firing the values of
     * URF_FRONT_CP_MASK; with urf_set_front_curb_points on top of that the same values at 16, 32 and 128 lasers (whether 128 lasers are
     * taken at all is lasers_ok's business).  9..30 keep the general kernels everywhere. */
    bool curb_points_ok(unsigned L, int cp) const { return cp == 5 || (front_mode == 3 && (L == 64u || curb_points) && cp >= 1 && cp <= 8 && ((URF_FRONT_CP_MASK >> cp) & 1u) != 0u); }
    /* the tiles per scan: urf_set_front_long_sweeps raises the limit in modes 2 and 3 (the finish kernels with more dynamic LDS) */
    uint32_t front_max_tiles() const { return long_sweeps && every_batch() ? URF_FRONT_LONG_MAX_TILES : URF_FRONT_MAX_TILES; }
    /* mode 1: the scans per batch call from which sweeps in firing order gain (16 / 32 lasers: never, until their crossover has been measured) */
    static uint32_t min_scans(unsigned L) { return L == 64u ? URF_FRONT_MIN_SCANS : (L == 32u ? URF_FRONT_MIN_SCANS_32 : URF_FRONT_MIN_SCANS_16); }
    /* Row-major sweeps gain at any batch size (the general kernels need 0.64 ms for four such sweeps, the fused ones 0.26, tools/r6_min_scans.py
     * --rows): once a scan has taken the layout, or while the sighting is on probation, batches below min_scans() and the callback path take the
     * fused kernels too.  (16 / 32 / 128 lasers: nothing below mode 2 -- no batch size, no row-major sighting, no callback path.) */
    bool small_ok(unsigned L) const { return front_rows && (rows_used || rows_probation > 0) && (L == 64u || every_batch()); }
    /* tiles per block of k_front: what URF_FRONT_TPB says, else by batch size; 128 lasers (lsh 7): an even number, because a presence word
     * of k_front128 covers two tiles and no block may end inside one */
    uint32_t tiles_per_block(uint32_t n_scans, uint32_t lsh) const
    {
        const uint32_t tpb = front_tpb ? front_tpb : (n_scans >= URF_FRONT_TPB_SCANS ? URF_FRONT_TPB_LARGE : (n_scans >= 16u ? URF_FRONT_TPB_SMALL : 1u));
        return lsh != 7u ? tpb : (tpb < 2u ? 2u : (tpb & ~1u));
    }

    /* the march of a fused call is, or would be, the multi-sector one (plan(): a.front_ms of a call that is fused) */
    bool ms_ok(const urf_dev_params& dp) const { return multi_sector && dp.p.star_shaped_method != 0 && (dp.p.curbPoints == 5 || multi_sector_cp); }

    /* The launch decisions of one call (a.tiles, a.capture, a.n_scans set): slot, a sweep of the callback path; general_only, no fused
     * kernels (last_call). */
    void plan(urf_kargs& a, const urf_dev_params& dp, bool slot, bool general_only) const
    {
        a.table_lookahead = speculate ? URF_TABLE_LOOKAHEAD : 0u;
        a.table_hint = (speculate && use_hint) ? 1u : 0u;
        /* A sweep of the callback path is waited for by the host before anybody sees its result: the kernels that normally find nothing
         * to do -- the two repair kernels behind the speculative ring table, the two for the work lists of oversized star sectors, 20 of a
         * sweep's 200 microseconds -- are left out, k_index voids a sweep that needed them, and urf_classify_pc2_wait() runs it again. */
        a.optimistic = slot ? ((speculate ? URF_OPT_NO_REPAIR : 0u) | (slot_lists ? 0u : URF_OPT_NO_LISTS) | (slot_nan ? 0u : URF_OPT_NO_NAN) |
                               (slot_ties ? 0u : URF_OPT_NO_TIES)) : 0u;
        /* The fused front end: a firing of 64, 32 or 16 lasers (params.channels) = the first lanes of a wave (128: two per lane), the
         * detectors' window of curbPoints points in registers (the instance is chosen per call: urf_front_family_of), no stage capture (its
         * values are the general kernels').  Sweeps in firing order gain from 192 per call on, and not as single sweeps of the callback path
         * (tools/r6_single_sweep.py); row-major ones always (small_ok). */
        const unsigned L = (unsigned)dp.p.channels;
        a.front_lsh = L == 16u ? 4u : (L == 32u ? 5u : (L == 128u ? 7u : 6u));
        const bool shape = front_mode != 0 && !front_off && !general_only && !want_ring_sorted && a.capture == 0 && lasers_ok(L) &&
                           curb_points_ok(L, dp.p.curbPoints) && a.tiles <= front_max_tiles();
        const bool enough = slot ? small_ok(L) : (every_batch() || small_ok(L) || a.n_scans >= min_scans(L));
        a.front = (shape && enough) ? 1u : 0u;
        a.front_sight = (shape && !a.front && !front_rows && !rows_oom && (L == 64u || every_batch())) ? 1u : 0u;
        a.front_tpb = tiles_per_block(a.n_scans, a.front_lsh);
        a.front_lists = (a.front && !front_direct && !slot) ? 1u : 0u;   /* (the callback path's sequence holds the general kernels as grids anyway) */
        a.front_rows = (a.front && front_rows) ? 1u : 0u;   /* (independent of the two other speculations: the repair kernels come with it) */
        a.front_ms = (a.front && multi_sector && dp.p.star_shaped_method != 0 && (dp.p.curbPoints == 5 || multi_sector_cp)) ? 1u : 0u;
    }

    /* Why plan() gave a call the general kernels, and what would give it the fused ones (urf_front_explain; a.tiles, a.capture, a.n_scans
     * set, as for plan()).  why: one URF_WHY_CALL_* bit per term of plan()'s `shape` and `enough` that is false, 0 exactly when plan() sets
     * a.front.  advice: the smallest set of URF_ADVICE_* that makes every one of them true -- the mode to raise to, the switches to turn
     * on, RESET (urf_set_front_mode again: forget_front and want_ring_sorted; a general_only run is the read-out's own and ends with it),
     * CAPTURE_OFF, BATCH (a sweep of the callback path as a batch call, which then is large enough: 512 scans) --; NEVER where no setting
     * helps, with the other bits still naming what else was missing.  FRONT_OUTPUTS goes with a sticky read-out: it does not undo it
     * (RESET does) but keeps the next read-out from doing it again.  Asks plan()'s questions, decides no launch. */
    struct reasons { uint32_t why, advice; };
    reasons why(const urf_kargs& a, const urf_dev_params& dp, bool slot, bool general_only) const
    {
        const unsigned L = (unsigned)dp.p.channels;
        const int cp = dp.p.curbPoints;
        uint32_t w = 0, adv = 0;
        int mode = front_mode;   /* the mode the advice raises to */
        if (front_mode == 0)
            w |= URF_WHY_CALL_MODE_OFF, mode = 2;   /* (no bit says 1: mode 2 takes every batch call mode 1 takes) */
        if (front_off)
            w |= URF_WHY_CALL_STOPPED, adv |= URF_ADVICE_RESET;
        if (general_only || want_ring_sorted) {
            w |= URF_WHY_CALL_READOUT, adv |= URF_ADVICE_RESET;
            if (!front_outputs)
                adv |= URF_ADVICE_FRONT_OUTPUTS;
        }
        if (a.capture != 0)
            w |= URF_WHY_CALL_CAPTURE, adv |= URF_ADVICE_CAPTURE_OFF;
        const bool known = L == 128u || L == 64u || L == 32u || L == 16u;
        if (!known)
            adv |= URF_ADVICE_NEVER;
        if (!lasers_ok(L)) {
            w |= URF_WHY_CALL_LASERS;
            if (L == 128u) {
                mode = mode < 2 ? 2 : mode;
                if (!lasers128)
                    adv |= URF_ADVICE_LASERS128;
            }
        }
        const bool cp_known = cp >= 1 && cp <= 8 && ((URF_FRONT_CP_MASK >> cp) & 1u) != 0u;
        if (!curb_points_ok(L, cp))
            w |= URF_WHY_CALL_CURB_POINTS;
        if (cp != 5 && cp_known) {   /* (asked of the mode the advice raises to: a call that lacks the mode for other reasons lacks it here too) */
            mode = 3;
            if (L != 64u && !curb_points)
                adv |= URF_ADVICE_CURB_POINTS;
            if (L == 128u && !lasers128)
                adv |= URF_ADVICE_LASERS128;
        } else if (cp != 5) {
            adv |= URF_ADVICE_NEVER;
        }
        if (a.tiles > front_max_tiles())
            w |= URF_WHY_CALL_TILES;
        if (a.tiles > URF_FRONT_LONG_MAX_TILES) {
            adv |= URF_ADVICE_NEVER;
        } else if (a.tiles > URF_FRONT_MAX_TILES) {
            mode = mode < 2 ? 2 : mode;
            if (!long_sweeps)
                adv |= URF_ADVICE_LONG_SWEEPS;
        }
        /* `enough`, asked of the mode so far: a mode raised for the shape's sake takes every batch call, and with a row-major sighting
         * the callback path as well */
        const bool sighted = front_rows && (rows_used || rows_probation > 0);
        if (!(slot ? small_ok(L) : (every_batch() || small_ok(L) || a.n_scans >= min_scans(L)))) {
            w |= slot ? URF_WHY_CALL_CALLBACK : URF_WHY_CALL_FEW_SCANS;
            if (!slot || sighted) {   /* (with the sighting all a sweep lacks is the mode: small_ok) */
                mode = mode < 2 ? 2 : mode;
            } else {
                adv |= URF_ADVICE_BATCH;
                if (mode < 2 && 512u < min_scans(L))
                    mode = 2;
            }
        }
        if (mode != front_mode)
            adv |= mode == 3 ? URF_ADVICE_MODE_3 : URF_ADVICE_MODE_2;
        return reasons{ w, w ? adv : 0u };
    }
};

/* The family of the fused front end a call's kernels belong to, from what plan() decided (a.front, a.front_lsh, a.front_rows, a.front_ms,
 * a.tiles) and the call's curbPoints.  urf_api.hip's table (front_kernels) turns it into the kernels; nothing else on the host knows
 * what differs between the families.  A call without the fused kernels: all zero. */
struct urf_front_family {
    uint8_t fused;          /* a.front */
    uint8_t lasers;         /* 0, 1, 2, 3: 16, 32, 64, 128 lasers per firing (the march: k_front16*, k_front32*, k_front*, k_front128*) */
    uint8_t wide;           /* 128 lasers: probe, transpose, finish and label kernel are the *128 siblings, the candidate lists likewise */
    uint8_t cp;             /* the march's and the finish kernel's instance: 5, or the call's curbPoints where it is one of URF_FRONT_CP_OTHERS */
    uint8_t ms;             /* the march is the k_front*_ms instance (a.front_ms), k_front*_ms_cp<n> where cp is not 5 */
    uint8_t rows;           /* the probe and the transpose are launched (a.front_rows) */
    uint32_t finish_tiles;  /* the tiles the finish kernel's dynamic LDS is sized for (128 lasers: an even number) */
};
static inline urf_front_family urf_front_family_of(uint32_t front, uint32_t front_lsh, uint32_t front_rows, uint32_t front_ms, uint32_t tiles, int cp)
{
    if (!front)
        return urf_front_family{ 0, 0, 0, 0, 0, 0, 0u };
#define URF_FRONT_CP_X(n) || cp == n
    const bool other = false URF_FRONT_CP_OTHERS(URF_FRONT_CP_X);
#undef URF_FRONT_CP_X
    const bool wide = front_lsh == 7u;
    return urf_front_family{ 1, (uint8_t)(front_lsh - 4u), wide, (uint8_t)(other ? cp : 5), front_ms != 0u, front_rows != 0u,
                             wide ? URF_FRONT128_TILES2(tiles) : tiles };
}

/* ---- the callback path's host decisions (urf_classify_pc2_async; tests/cpp/policy_sweep.cpp) ----
 * The shape a sweep runs as and the bytes to ask its slot's message buffers for (cap: what the smaller of them holds).  urf_set_sweep_quantum:
 * the sweep runs as the next multiple of the quantum, (NaN, NaN, NaN) behind its own points -- the reference drops non-finite points before
 * anything else -- and every sweep of that padded length replays one captured sequence; beyond max_points: unpadded, under its own key. */
struct urf_sweep_dims { uint32_t n_run; bool pad; size_t want; };   /* the points it runs as | in a padded sequence | bytes for slot_prepare */
static inline urf_sweep_dims urf_sweep_shape(uint32_t n_points, uint32_t point_step, uint32_t quantum, uint32_t max_points, bool planes, size_t cap)
{
    uint32_t n_run = n_points;
    bool pad = false;
    if (const uint32_t q = quantum) {
        const uint64_t up = ((uint64_t)n_points + q - 1) / q * q;
        if (up <= max_points) {
            n_run = (uint32_t)up;
            pad = true;   /* (a multiple of the quantum too: it shares the padded sequence of its length) */
        }
    }
    const size_t bytes = (size_t)n_points * point_step;
    const size_t n4 = ((size_t)n_run + 3) & ~(size_t)3;
    const size_t plane_bytes = 3 * sizeof(float) * n4;
    size_t want = planes && plane_bytes > bytes ? plane_bytes : bytes;
    if (pad && want > cap) {
        /* a new buffer forgets the slot's sequences, and the messages of such a stream keep growing by a few points: room for twice the
         * padded length (at most max_points), so that the lengths to come fit the buffer this one gets */
        const size_t room = std::min<size_t>(2 * (size_t)n_run, max_points);
        want = std::max(want, ((room + 3) & ~(size_t)3) * std::max<size_t>(point_step, 3 * sizeof(float)));
    }
    return urf_sweep_dims{ n_run, pad, want };
}

/* A slot's captured launch sequences as the host decides about them: entry i is live (captured into), was built for key[3] = { epoch,
 * n_run << 32 | point_step, the offsets } and ran last at `used` (urf_ctx::seq_clock); graph and run: urf_ctx::slot_t::seqs[i]. */
struct urf_seq_cache {
    struct entry { bool live = false; uint64_t key[3] = { 0, 0, 0 }, used = 0; } e[URF_SWEEP_SEQS];
    void take(unsigned i, const uint64_t* key) { e[i] = entry{ true, { key[0], key[1], key[2] }, 0 }; }
    void drop(unsigned i) { e[i] = entry{}; }
    /* the sequences are no sweep's any more (a new message buffer, the other staging format): the slot's next submission drops them */
    void invalidate() { for (entry& q : e) q.key[0] = 0; }
    /* The entry a sweep of `key` runs from.  release(i), which ends in drop(i), is called for every entry of another epoch, whatever its key;
     * hit = false: the caller releases, captures into and take()s the one returned -- the first free of the first n_seqs, else their LRU. */
    template <class F>
    unsigned acquire(const uint64_t* key, unsigned n_seqs, bool& hit, F&& release)
    {
        unsigned at = 0;
        hit = false;
        for (unsigned i = 0; i < URF_SWEEP_SEQS; i++) {
            if (e[i].live && e[i].key[0] != key[0])
                release(i);
            if (e[i].live && e[i].key[1] == key[1] && e[i].key[2] == key[2]) {
                at = i;
                hit = true;
            }
        }
        for (unsigned i = 0; !hit && i < n_seqs && e[at].live; i++)   /* (no entry holds the key: room) */
            if (!e[i].live || e[i].used < e[at].used)
                at = i;
        return at;
    }
    /* the sequences a sweep of `epoch` can still replay (urf_callback_path_captures) */
    unsigned resident(uint64_t epoch) const
    {
        unsigned n = 0;
        for (const entry& q : e)
            n += (q.live && q.key[0] == epoch) ? 1u : 0u;
        return n;
    }
};

#endif /* URF_POLICY_HPP */
