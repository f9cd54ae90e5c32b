// env.h — the environment switches of libwgbsseg.so and the one way to read them (no HIP here: stitch.h and its host tests use it too).
//
// All optional; the defaults are what the measurements use.  "create": read when a context is created (wgbsseg_create, every share of
// wgbsseg_group_create) — set it before; "upload": per upload call; "batch": per batch, on a live context; "call": per API call;
// "process": once, on first use.  DESIGN.md 4 has the longer account of what each is for.
//
//   WGBSSEG_...              default        accepted                     read     what for
//   COST_BUDGET_MB           6144           > 0, else the default        create   cap of the scored-block buffer per stage
//   FORCE_STAGES             0              any                          create   exactly this many recurrence stages (tests, share sweeps)
//   STAGE_GATE               768            clamped to >= 0              create   tiles of slack at which k_stage_gate opens; 0: one scoring stream, no gate
//   STAGE_GATE_SHARED        0              flag                         create   gate whatever the tiles, and beside other contexts on the device (tests)
//   STAGE_GATE_WIDE_EVALS    100000         any                          create   evaluations per step from which a job with medium / wide tiles is gated
//   STAGE_MIN_EVALS          21000          any                          create   evaluations per step of the longest chunk from which few chunks are staged
//   LAST_STAGE_PCT           per job        clamped to 5..800            create   length of a staged job's last stage in percent of the others' (A/B, tests)
//   DP_MODE                  0              clamped to 0..2              create   1: 32-step batches (wide-window path), 2: the same with 15 worker waves
//   DP_WLEAN                 1              flag                         create   0: the narrow batches of a wide job on k_dp's generic step
//   NS, TI                   0              any                          create   force the samples per LDS group / the narrow tile width (tests, tuning)
//   BLOCK_SUMS_GENERAL       0              flag                         create   1: never the streaming block-sums kernel
//   DIV_SHORT                1              flag                         create   0: always the 8-instruction division core
//   SCAN_PIECE_SITES         4096           >= 1024, cut to k * 1024     create   sites per wave task of k_validate
//   MEDIUM_WMAX              WG_MEDIUM_WMAX clamped to 0..the default    create   widest window of a medium tile; at most the narrow tiles': no medium class
//   NO_EARLY                 0              flag                         create   1: the first batch of a region-level call delivers everything at once
//   NO_SPECULATION           0              flag                         create   1: junction patches only when the reference would ask for them
//   PROFILE                  0              0, 1, 2                      process  1: host time of a call (allocations, uploads, destroy) on stderr;
//                                                                        + create 2: also every batch's device time line and host clock
//   UPLOAD_PIN               1              flag                         create   0: the upload threads run where the scheduler puts them
//   UPLOAD_PIECE_KB          see below      >= 64, else the default      upload   staging piece: 4 MB blocking; streaming 1 MB, 2 MB from 4 GB up
//   UPLOAD_THREADS           see below      > 0, else the default; <= 64 upload   4; streaming 8 from 4 GB up (then cut to the work there is)
//   UPLOAD_DEPTH             2              2..8, else the default       upload   staging pieces (copies in flight) per thread; streaming form only
//   UPLOAD_POPULATE          1              flag                         upload   0: a fault per page instead of one madvise per piece; streaming form only
//   UPLOAD_NT                1              flag                         upload   0: memcpy instead of the non-temporal fill; streaming form only
//   PLAIN_RING_ROWS          ~1 GB of rows  > 0, raised to the window    batch    cap of the plain path's ring of rows (tests: the banded ring)
//   DP_DEBUG                 0              any                          batch    builds with -DWGBSSEG_DP_TIMING only: k_dp's timing modes (WRONG results)
//   STITCH_THREADS           min(8,cores/2) clamped to >= 1              process  host threads of the stitching pool (1: everything on the caller)
//   PROFILE_STITCH           0              flag                         call     host phases of the stitching on stderr
//   PAIR_CORNERS             0              flag                         call     1: k_pair_hist counts the two corner cells in registers, not through LDS atomics (A/B, tests)
#pragma once
#include <climits>
#include <cstdlib>

// unset: def; a number (atoll / atof: text that is none counts as 0), with bounds clamped into [lo, hi]
inline long long env_int(const char* name, long long def, long long lo = LLONG_MIN, long long hi = LLONG_MAX)
{
    const char* e = getenv(name);
    const long long v = e ? atoll(e) : def;
    return v < lo ? lo : v > hi ? hi : v;
}
inline double env_double(const char* name, double def) { const char* e = getenv(name); return e ? atof(e) : def; }
inline bool env_flag(const char* name, bool def) { const char* e = getenv(name); return e ? atoll(e) != 0 : def; }
