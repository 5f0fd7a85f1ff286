/*
 * policy_table.cpp -- urf_policy::plan and urf_front_family_of (urban_road_filter_amd/csrc/urf_policy.hpp) over a fixed cross product of
 * policy states and calls, without HIP and without a GPU:   g++ -std=c++17 -O2 -I include -I urban_road_filter_amd/csrc
 *
 *   policy_table                                one line per (front_mode, channels) slice: "MODE:CHANNELS rows fnv1a-64", and one for
 *                                               the block of the ring table's speculation and the callback path's short sequence ("spec")
 *   policy_table --rows SLICE [name=value ...]  the slice's rows as text, fixed width (two header lines: the names, the widths), only
 *                                               the rows whose inputs have the values given
 *
 * The checksum runs over every output field of every row, in enumeration order (the last variable fastest); tests/golden/policy_table.json
 * holds what the parent of the commit that added this file decided (tests/test_policy_table.py).
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "urf_policy.hpp"

namespace {

struct Var {
    const char* name;
    int n;
    int values[8];
};
/* rows_state: 0 never sighted, 1 sighted and on probation, 2 sighted and used, 3 sighted and lapsed, 4 rows_oom */
enum { FRONT_MODE, CHANNELS, LASERS128, CURB_POINTS, MULTI_SECTOR, LONG_SWEEPS, WANT_RING_SORTED, FRONT_OFF, FRONT_DIRECT, FRONT_TPB, ROWS_STATE,
       CP, STAR, TILES, N_SCANS, CAPTURE, SLOT, GENERAL_ONLY, N_IN };
const Var IN[N_IN] = {
    { "front_mode", 4, { 0, 1, 2, 3 } },
    { "channels", 5, { 8, 16, 32, 64, 128 } },
    { "lasers128", 2, { 0, 1 } },
    { "curb_points", 2, { 0, 1 } },
    { "multi_sector", 2, { 0, 1 } },
    { "long_sweeps", 2, { 0, 1 } },
    { "want_ring_sorted", 2, { 0, 1 } },
    { "front_off", 2, { 0, 1 } },
    { "front_direct", 2, { 0, 1 } },
    { "front_tpb", 3, { 0, 1, 3 } },
    { "rows_state", 5, { 0, 1, 2, 3, 4 } },
    { "curbPoints", 5, { 1, 4, 5, 8, 9 } },
    { "star_shaped_method", 2, { 0, 1 } },
    { "tiles", 6, { 1, 2, 128, 129, 256, 257 } },
    { "n_scans", 7, { 1, 15, 16, 191, 192, 511, 512 } },
    { "capture", 2, { 0, 1 } },
    { "slot", 2, { 0, 1 } },
    { "general_only", 2, { 0, 1 } },
};
/* the second block: its own inputs in front of `slot` */
enum { SPECULATE, USE_HINT, SLOT_LISTS, SLOT_NAN, SLOT_TIES, SPEC_SLOT, N_SPEC };
const Var SPEC[N_SPEC] = {
    { "speculate", 2, { 0, 1 } }, { "use_hint", 2, { 0, 1 } }, { "slot_lists", 2, { 0, 1 } },
    { "slot_nan", 2, { 0, 1 } }, { "slot_ties", 2, { 0, 1 } }, { "slot", 2, { 0, 1 } },
};
enum { O_FRONT, O_SIGHT, O_TPB, O_LISTS, O_ROWS, O_MS, O_LSH, O_LOOKAHEAD, O_HINT, O_OPTIMISTIC,
       O_FAM_FUSED, O_FAM_LASERS, O_FAM_WIDE, O_FAM_CP, O_FAM_MS, O_FAM_ROWS, O_FAM_FINISH_TILES, N_OUT };
const char* const OUT[N_OUT] = { "front", "front_sight", "front_tpb", "front_lists", "front_rows", "front_ms", "front_lsh", "table_lookahead",
                                 "table_hint", "optimistic", "fam.fused", "fam.lasers", "fam.wide", "fam.cp", "fam.ms", "fam.rows",
                                 "fam.finish_tiles" };

/* the columns of --rows: every value right-aligned in its width, one space between two */
int in_width(int k) { return k == TILES || k == N_SCANS || k == CHANNELS ? 3 : 1; }
int out_width(int k) { return k == O_LOOKAHEAD ? 4 : (k == O_FAM_FINISH_TILES ? 3 : (k == O_OPTIMISTIC ? 2 : 1)); }

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    uint64_t rows = 0;
    void byte(uint32_t b) { h = (h ^ (b & 0xffu)) * 0x100000001b3ull; }
    /* a row's output fields in ten bytes: the six flags of plan(), front_tpb, front_lsh, table_lookahead (two), optimistic, the family's
     * four flags with its laser index, its cp, its finish_tiles (two) */
    void row(const uint32_t* o)
    {
        byte(o[O_FRONT] | o[O_SIGHT] << 1 | o[O_LISTS] << 2 | o[O_ROWS] << 3 | o[O_MS] << 4 | o[O_HINT] << 5);
        byte(o[O_TPB]), byte(o[O_LSH]), byte(o[O_LOOKAHEAD]), byte(o[O_LOOKAHEAD] >> 8), byte(o[O_OPTIMISTIC]);
        byte(o[O_FAM_FUSED] | o[O_FAM_WIDE] << 1 | o[O_FAM_MS] << 2 | o[O_FAM_ROWS] << 3 | o[O_FAM_LASERS] << 4);
        byte(o[O_FAM_CP]), byte(o[O_FAM_FINISH_TILES]), byte(o[O_FAM_FINISH_TILES] >> 8);
        rows++;
    }
};

void outputs(const urf_policy& p, urf_kargs& a, const urf_dev_params& dp, bool slot, bool general_only, uint32_t* o)
{
    p.plan(a, dp, slot, general_only);
    const urf_front_family f = urf_front_family_of(a.front, a.front_lsh, a.front_rows, a.front_ms, a.tiles, dp.p.curbPoints);
    o[O_FRONT] = a.front, o[O_SIGHT] = a.front_sight, o[O_TPB] = a.front_tpb, o[O_LISTS] = a.front_lists, o[O_ROWS] = a.front_rows;
    o[O_MS] = a.front_ms, o[O_LSH] = a.front_lsh, o[O_LOOKAHEAD] = a.table_lookahead, o[O_HINT] = a.table_hint, o[O_OPTIMISTIC] = a.optimistic;
    o[O_FAM_FUSED] = f.fused, o[O_FAM_LASERS] = f.lasers, o[O_FAM_WIDE] = f.wide, o[O_FAM_CP] = f.cp, o[O_FAM_MS] = f.ms, o[O_FAM_ROWS] = f.rows;
    o[O_FAM_FINISH_TILES] = f.finish_tiles;
}

/* the next combination of vars[first..n), the last one fastest (v: its values); false after the last */
bool next(const Var* vars, int first, int n, int* idx, int* v)
{
    for (int k = n - 1; k >= first; k--) {
        if (++idx[k] == vars[k].n)
            idx[k] = 0;
        v[k] = vars[k].values[idx[k]];
        if (idx[k])
            return true;
    }
    return false;
}

urf_kargs g_a;   /* (zero: plan() writes what it decides, the walk what plan() reads) */
urf_dev_params g_dp;

/* right-aligned in `width` characters and a space behind it */
void put(std::string& line, unsigned value, int width)
{
    char buf[12];
    for (int k = width - 1; k >= 0; k--, value /= 10u)
        buf[k] = value || k == width - 1 ? (char)('0' + value % 10u) : ' ';
    buf[width] = ' ';
    line.append(buf, (size_t)width + 1);
}

/* the rows of `vars` (IN, or IN with some variables narrowed to one value) from the first combination on: checksum, or text */
Fnv walk(const Var* vars, bool print)
{
    Fnv sum;
    int idx[N_IN] = { 0 }, v[N_IN];
    for (int k = 0; k < N_IN; k++)
        v[k] = vars[k].values[0];
    std::string line;
    do {
        urf_policy p;
        p.front_mode = v[FRONT_MODE];
        p.lasers128 = v[LASERS128], p.curb_points = v[CURB_POINTS], p.multi_sector = v[MULTI_SECTOR], p.long_sweeps = v[LONG_SWEEPS];
        p.want_ring_sorted = v[WANT_RING_SORTED], p.front_off = v[FRONT_OFF], p.front_direct = v[FRONT_DIRECT];
        p.front_tpb = (uint32_t)v[FRONT_TPB];
        const int rs = v[ROWS_STATE];
        p.front_rows = rs >= 1 && rs <= 3, p.rows_used = rs == 2, p.rows_probation = rs == 1 ? 16u : 0u, p.rows_oom = rs == 4;
        g_dp.p.channels = v[CHANNELS], g_dp.p.curbPoints = v[CP], g_dp.p.star_shaped_method = v[STAR];
        g_a.tiles = (uint32_t)v[TILES], g_a.n_scans = (uint32_t)v[N_SCANS], g_a.capture = (uint32_t)v[CAPTURE];
        uint32_t o[N_OUT];
        outputs(p, g_a, g_dp, v[SLOT] != 0, v[GENERAL_ONLY] != 0, o);
        sum.row(o);
        if (print) {
            line.clear();
            for (int k = 0; k < N_IN; k++)
                put(line, (unsigned)v[k], in_width(k));
            for (int k = 0; k < N_OUT; k++)
                put(line, o[k], out_width(k));
            line.back() = '\n';
            fwrite(line.data(), 1, line.size(), stdout);
        }
    } while (next(vars, 0, N_IN, idx, v));
    return sum;
}

/* IN with variable k narrowed to the one value */
void narrow(Var* vars, int k, int value)
{
    vars[k].n = 1;
    vars[k].values[0] = value;
}

Fnv spec_block(bool print)
{
    Fnv sum;
    int idx[N_SPEC] = { 0 }, v[N_SPEC] = { 0 };
    g_dp.p.channels = 64, g_dp.p.curbPoints = 5, g_dp.p.star_shaped_method = 1;
    g_a.tiles = 2, g_a.n_scans = 1, g_a.capture = 0;
    do {
        urf_policy p;
        p.speculate = v[SPECULATE], p.use_hint = v[USE_HINT], p.slot_lists = v[SLOT_LISTS], p.slot_nan = v[SLOT_NAN], p.slot_ties = v[SLOT_TIES];
        uint32_t o[N_OUT];
        outputs(p, g_a, g_dp, v[SPEC_SLOT] != 0, false, o);
        sum.row(o);
        if (print) {
            for (int k = 0; k < N_SPEC; k++)
                printf("%d ", v[k]);
            for (int k = 0; k < N_OUT; k++)
                printf("%u%s", o[k], k + 1 < N_OUT ? " " : "\n");
        }
    } while (next(SPEC, 0, N_SPEC, idx, v));
    return sum;
}

int usage()
{
    fprintf(stderr, "usage: policy_table [--rows MODE:CHANNELS|spec [name=value ...]]\n");
    return 2;
}

}   // namespace

int main(int argc, char** argv)
{
    if (argc == 1) {
        for (int m = 0; m < IN[FRONT_MODE].n; m++)
            for (int c = 0; c < IN[CHANNELS].n; c++) {
                Var vars[N_IN];
                memcpy(vars, IN, sizeof vars);
                narrow(vars, FRONT_MODE, IN[FRONT_MODE].values[m]);
                narrow(vars, CHANNELS, IN[CHANNELS].values[c]);
                const Fnv s = walk(vars, false);
                printf("%d:%d %llu %016llx\n", IN[FRONT_MODE].values[m], IN[CHANNELS].values[c], (unsigned long long)s.rows, (unsigned long long)s.h);
            }
        const Fnv s = spec_block(false);
        printf("spec %llu %016llx\n", (unsigned long long)s.rows, (unsigned long long)s.h);
        return 0;
    }
    if (argc < 3 || strcmp(argv[1], "--rows") != 0)
        return usage();
    if (strcmp(argv[2], "spec") == 0) {
        printf("#");
        for (int k = 0; k < N_SPEC; k++)
            printf(" %s", SPEC[k].name);
        for (int k = 0; k < N_OUT; k++)
            printf(" %s", OUT[k]);
        printf("\n");
        spec_block(true);
        return 0;
    }
    int m = 0, c = 0;
    if (sscanf(argv[2], "%d:%d", &m, &c) != 2)
        return usage();
    Var vars[N_IN];
    memcpy(vars, IN, sizeof vars);
    narrow(vars, FRONT_MODE, m);
    narrow(vars, CHANNELS, c);
    for (int i = 3; i < argc; i++) {
        const char* eq = strchr(argv[i], '=');
        int k = 0;
        while (eq && k < N_IN && std::string(argv[i], (size_t)(eq - argv[i])) != IN[k].name)
            k++;
        if (!eq || k == N_IN)
            return usage();
        narrow(vars, k, atoi(eq + 1));
    }
    for (int k = 0; k < N_IN; k++) {   /* (only values of the product) */
        bool known = false;
        for (int j = 0; j < IN[k].n; j++)
            known = known || IN[k].values[j] == vars[k].values[0];
        if (vars[k].n == 1 && !known)
            return usage();
    }
    printf("#");
    for (int k = 0; k < N_IN; k++)
        printf(" %s", IN[k].name);
    for (int k = 0; k < N_OUT; k++)
        printf(" %s", OUT[k]);
    printf("\n# widths");
    for (int k = 0; k < N_IN; k++)
        printf(" %d", in_width(k));
    for (int k = 0; k < N_OUT; k++)
        printf(" %d", out_width(k));
    printf("\n");
    walk(vars, true);
    return 0;
}
