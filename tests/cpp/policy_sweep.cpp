/*
 * policy_sweep.cpp -- the callback path's two host decisions that need no HIP (urban_road_filter_amd/csrc/urf_policy.hpp), without a GPU:
 *   g++ -std=c++17 -O2 -I include -I urban_road_filter_amd/csrc
 *
 * urf_sweep_shape: the points a sweep runs as under urf_set_sweep_quantum (n_run, pad) and the bytes its slot's buffers are asked for
 * (want), "room for twice the padded length" included.  urf_seq_cache: a slot's captured sequences as {live, key, used} -- which
 * entries an epoch change drops, which entry a key finds, which one makes room: acquire(), called here the way sweep_sequence
 * (urf_api_sweep.hpp) calls it.
 *   policy_sweep                       prints "checks N failures 0" and returns 0, or the failing checks and 1
 *   policy_sweep lengths Q MAX A B     prints "n n_run pad" for every n in [A, B): tests/test_policy_sweep.py compares with its own rule
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "urf_policy.hpp"

namespace {

int g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        g_checks++;                                                    \
        if (!(cond)) {                                                 \
            g_failures++;                                              \
            std::printf("line %d: %s\n", __LINE__, #cond);             \
        }                                                              \
    } while (0)

const uint32_t Q = 2048u;
const size_t FITS = (size_t)1 << 30;   /* a buffer that already fits everything below */

bool is(const urf_sweep_dims& d, uint32_t n_run, bool pad, size_t want) { return d.n_run == n_run && d.pad == pad && d.want == want; }

void shapes()
{
    /* quantum 0: the sweep as it is; planes of n rounded up to 4 where they are larger than the records */
    CHECK(is(urf_sweep_shape(4001, 32, 0, 65536, false, 0), 4001, false, 4001u * 32u));
    CHECK(is(urf_sweep_shape(4001, 32, 0, 65536, true, 0), 4001, false, 4001u * 32u));
    CHECK(is(urf_sweep_shape(4001, 12, 0, 65536, true, 0), 4001, false, 4004u * 12u));
    CHECK(is(urf_sweep_shape(4001, 12, 0, 65536, false, FITS), 4001, false, 4001u * 12u));
    CHECK(is(urf_sweep_shape(1, 4, 0, 1, true, 0), 1, false, 48u));
    /* k q - 1, k q, k q + 1 points: a multiple of the quantum shares the padded sequence of its length */
    for (uint32_t k = 1; k <= 3; k++) {
        CHECK(is(urf_sweep_shape(k * Q - 1, 32, Q, 65536, false, FITS), k * Q, true, (size_t)(k * Q - 1) * 32u));
        CHECK(is(urf_sweep_shape(k * Q, 32, Q, 65536, false, FITS), k * Q, true, (size_t)k * Q * 32u));
        CHECK(is(urf_sweep_shape(k * Q + 1, 32, Q, 65536, false, FITS), (k + 1) * Q, true, (size_t)(k * Q + 1) * 32u));
    }
    /* a padded length of exactly max_points; one tile beyond it: unpadded, under its own length */
    CHECK(is(urf_sweep_shape(3 * Q - 5, 16, Q, 3 * Q, false, FITS), 3 * Q, true, (size_t)(3 * Q - 5) * 16u));
    CHECK(is(urf_sweep_shape(3 * Q, 16, Q, 3 * Q, false, FITS), 3 * Q, true, (size_t)3 * Q * 16u));
    CHECK(is(urf_sweep_shape(2 * Q + 1, 16, 2 * Q, 3 * Q, false, FITS), 2 * Q + 1, false, (size_t)(2 * Q + 1) * 16u));   /* (4 Q = max_points + one tile) */
    CHECK(is(urf_sweep_shape(2 * Q + 1, 16, 2 * Q, 3 * Q, true, 0), 2 * Q + 1, false, (size_t)(2 * Q + 1) * 16u));       /* (no pad: no extra room either) */
    CHECK(is(urf_sweep_shape(3 * Q + 9, 32, Q, 3 * Q + 100, false, 0), 3 * Q + 9, false, (size_t)(3 * Q + 9) * 32u));
    /* point_step 12, 16 and 32, staged as planes and as records, in a buffer that fits: the planes are those of the PADDED length */
    CHECK(is(urf_sweep_shape(4000, 12, Q, 65536, true, FITS), 4096, true, 4096u * 12u));
    CHECK(is(urf_sweep_shape(4000, 12, Q, 65536, false, FITS), 4096, true, 4000u * 12u));
    CHECK(is(urf_sweep_shape(4000, 16, Q, 65536, true, FITS), 4096, true, 4000u * 16u));
    CHECK(is(urf_sweep_shape(4000, 16, Q, 65536, false, FITS), 4096, true, 4000u * 16u));
    CHECK(is(urf_sweep_shape(4000, 32, Q, 65536, true, FITS), 4096, true, 4000u * 32u));
    CHECK(is(urf_sweep_shape(4000, 32, Q, 65536, false, FITS), 4096, true, 4000u * 32u));
    CHECK(is(urf_sweep_shape(4090, 12, Q, 65536, true, 4096u * 12u), 4096, true, 4096u * 12u));   /* (exactly the buffer: fits) */
    /* ... and in one that does not: room for min(2 n_run, max_points) points, rounded up to 4, of max(point_step, 12) bytes */
    CHECK(is(urf_sweep_shape(4000, 12, Q, 65536, true, 0), 4096, true, 8192u * 12u));
    CHECK(is(urf_sweep_shape(4000, 12, Q, 65536, false, 4000u * 12u - 1u), 4096, true, 8192u * 12u));
    CHECK(is(urf_sweep_shape(4000, 16, Q, 65536, true, 0), 4096, true, 8192u * 16u));
    CHECK(is(urf_sweep_shape(4000, 32, Q, 65536, false, 0), 4096, true, 8192u * 32u));
    CHECK(is(urf_sweep_shape(4000, 32, Q, 65536, true, 127999u), 4096, true, 8192u * 32u));
    CHECK(is(urf_sweep_shape(4000, 4, Q, 65536, true, 0), 4096, true, 8192u * 12u));       /* (a record shorter than its three plane words) */
    CHECK(is(urf_sweep_shape(4000, 32, Q, 6144, false, 0), 4096, true, 6144u * 32u));      /* (at most max_points) */
    CHECK(is(urf_sweep_shape(4000, 32, Q, 6146, false, 0), 4096, true, 6148u * 32u));      /* (rounded up to 4) */
    CHECK(is(urf_sweep_shape(4000, 32, Q, 4096, false, 0), 4096, true, 4096u * 32u));
    CHECK(is(urf_sweep_shape(6000, 64, Q, 6144, false, 0), 6144, true, 6144u * 64u));
    CHECK(is(urf_sweep_shape(4000, 32, 0, 65536, false, 0), 4000, false, 4000u * 32u));    /* (quantum off: what the message needs) */
}

/* the live entry that holds the key's sequence, -1: none (what acquire would hit, without acquiring) */
int find(const urf_seq_cache& c, uint64_t epoch, uint64_t k1, uint64_t k2)
{
    int at = -1;
    for (unsigned i = 0; i < URF_SWEEP_SEQS; i++)
        if (c.e[i].live && c.e[i].key[0] == epoch && c.e[i].key[1] == k1 && c.e[i].key[2] == k2)
            at = (int)i;
    return at;
}

/* one submission as sweep_sequence runs it: acquire -- a released entry's graph would be destroyed there --, capture and take on a miss,
 * the clock */
struct Slot {
    urf_seq_cache cache;
    uint64_t clock = 0;
    unsigned captured = 0, dropped = 0;
    int submit(uint64_t epoch, uint64_t k1, uint64_t k2, unsigned n_seqs)
    {
        const uint64_t key[3] = { epoch, k1, k2 };
        bool hit;
        const unsigned at = cache.acquire(key, n_seqs, hit, [&](unsigned i) {
            cache.drop(i);
            dropped++;
        });
        if (!hit) {
            dropped += cache.e[at].live ? 1u : 0u;
            cache.drop(at);
            cache.take(at, key);
            captured++;
        }
        cache.e[at].used = ++clock;
        return (int)at;
    }
    unsigned live() const
    {
        unsigned n = 0;
        for (const auto& q : cache.e)
            n += q.live ? 1u : 0u;
        return n;
    }
};

void sequences()
{
    {   /* one sequence per slot: a second key replaces the first */
        Slot s;
        CHECK(s.cache.resident(1) == 0 && find(s.cache, 1, 10, 0) == -1);
        CHECK(s.submit(1, 10, 0, 1) == 0 && s.captured == 1);
        CHECK(s.submit(1, 10, 0, 1) == 0 && s.captured == 1);   /* (a hit) */
        CHECK(s.submit(1, 11, 0, 1) == 0 && s.captured == 2 && s.dropped == 1);
        CHECK(find(s.cache, 1, 10, 0) == -1 && find(s.cache, 1, 11, 0) == 0);
        CHECK(s.submit(1, 11, 7, 1) == 0 && s.captured == 3);   /* (the third word is part of the key) */
        CHECK(s.live() == 1 && s.cache.resident(1) == 1);
    }
    {   /* URF_SWEEP_SEQS: free entries in order, then the least recently used; a hit refreshes `used` */
        Slot s;
        for (unsigned k = 0; k < URF_SWEEP_SEQS; k++)
            CHECK(s.submit(1, 100 + k, 0, URF_SWEEP_SEQS) == (int)k);
        CHECK(s.captured == URF_SWEEP_SEQS && s.dropped == 0 && s.cache.resident(1) == URF_SWEEP_SEQS);
        CHECK(s.submit(1, 100, 0, URF_SWEEP_SEQS) == 0 && s.captured == URF_SWEEP_SEQS);   /* the oldest one, used again */
        CHECK(s.submit(1, 200, 0, URF_SWEEP_SEQS) == 1 && s.dropped == 1);                 /* ... so the second oldest goes */
        CHECK(find(s.cache, 1, 100, 0) == 0 && find(s.cache, 1, 101, 0) == -1);
        CHECK(s.submit(1, 201, 0, URF_SWEEP_SEQS) == 2 && s.submit(1, 101, 0, URF_SWEEP_SEQS) == 3);
        CHECK(s.cache.resident(1) == URF_SWEEP_SEQS && s.live() == URF_SWEEP_SEQS);
        /* the quantum turned off with the epoch it bumps: one entry again, the first */
        CHECK(s.cache.resident(2) == 0);
        CHECK(s.submit(2, 100, 0, 1) == 0 && s.live() == 1 && s.cache.resident(2) == 1 && s.dropped == 3 + URF_SWEEP_SEQS);
    }
    {   /* an epoch change drops every live entry whatever its key; a free entry in the middle is found first */
        Slot s;
        for (unsigned k = 0; k < 5; k++)
            s.submit(7, k, k, URF_SWEEP_SEQS);
        CHECK(s.cache.resident(7) == 5 && s.cache.resident(8) == 0 && s.live() == 5);   /* (what urf_callback_path_captures reports before the next sweep) */
        CHECK(s.submit(8, 3, 3, URF_SWEEP_SEQS) == 0 && s.captured == 6 && s.dropped == 5 && s.live() == 1);
        s.submit(8, 4, 4, URF_SWEEP_SEQS);
        s.submit(8, 5, 5, URF_SWEEP_SEQS);
        s.cache.drop(1);
        CHECK(s.cache.resident(8) == 2 && s.submit(8, 6, 6, URF_SWEEP_SEQS) == 1);
        /* a new buffer, or the other staging format: the sequences are nobody's any more, the next submission releases them */
        s.cache.invalidate();
        CHECK(s.cache.resident(8) == 0 && s.live() == 3);
        CHECK(s.submit(8, 4, 4, URF_SWEEP_SEQS) == 0 && s.live() == 1 && s.cache.resident(8) == 1);
    }
    {   /* resident: live entries of the epoch, summed over the slots as urf_callback_path_captures sums them */
        Slot slots[4];
        unsigned want = 0;
        for (unsigned i = 0; i < 4; i++)
            for (unsigned k = 0; k <= i; k++, want++)
                slots[i].submit(3, k, 0, URF_SWEEP_SEQS);
        unsigned got = 0, captured = 0;
        for (const Slot& s : slots) {
            got += s.cache.resident(3);
            captured += s.captured;
        }
        CHECK(got == want && captured == want && want == 10);
    }
}

}   // namespace

int main(int argc, char** argv)
{
    if (argc == 6 && !std::strcmp(argv[1], "lengths")) {
        const uint32_t q = (uint32_t)std::strtoul(argv[2], nullptr, 10), max_points = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        for (uint32_t n = (uint32_t)std::strtoul(argv[4], nullptr, 10); n < (uint32_t)std::strtoul(argv[5], nullptr, 10); n++) {
            const urf_sweep_dims d = urf_sweep_shape(n, 32, q, max_points, false, 0);
            std::printf("%u %u %d\n", n, d.n_run, d.pad ? 1 : 0);
        }
        return 0;
    }
    shapes();
    sequences();
    std::printf("checks %d failures %d\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
