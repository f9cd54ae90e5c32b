// view_plan.h — the host plan of `wgbstools view` (wgbsseg_patview_*): the argument checks with their messages, the limits of the
// record table and its arena, how the two grow, the sort's run length and number of merge passes, the slabs of the fetch, and the table
// of file boundaries of a view over several files (`wgbstools merge`) with the messages that name a file, and the labels and sources of
// `wgbstools mix_pat`: the checks of the names, their ranks, the table the device takes, the checks of a file's source.  No HIP
// here (like frag_plan.h): g++ compiles it alone, tests/native/view_host.cpp hands it to the tests.
//
// Limits.  A record is 32 bytes (view_core.h); their number stays below 2^31, so a permutation entry is a uint32.  A survivor puts
// its chromosome and at most its pattern into the arena, both bytes of its own line: the arena never holds more than the text fed,
// and room for "the bytes fed so far + this chunk" is always enough — no count from the device is needed to size it.  A valid line
// has at least WG_VIEW_MIN_LINE bytes, which bounds the records a chunk can add.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "block_plan.h"                // wg_plan_refuse
#include "view_core.h"

#define WG_VIEW_MAX_RECORDS 0x7fffffffLL
#define WG_VIEW_MIN_LINE 7               // "\t1\tC\t1\n": the shortest line that parses
#define WG_VIEW_MAX_CHUNK 0x7fffffffLL   // bytes of one chunk: lengths inside it fit 32 bits
#define WG_VIEW_DEFAULT_RECORDS (1 << 20)
#define WG_VIEW_RUN 512                  // R: indices one workgroup sorts in LDS
#define WG_VIEW_MERGE_ITEMS 16           // output elements one thread merges
#define WG_VIEW_SLAB (8ll << 20)         // bytes of one fetch through the page-locked staging buffer

struct ViewPlan {
    int64_t s = 1, e = 2;
    int flags = 0;
    int64_t min_len = 1;
    int64_t initial_records = WG_VIEW_DEFAULT_RECORDS;
};

inline int plan_view(int64_t s, int64_t e, int32_t flags, int32_t min_len, int64_t initial_records, ViewPlan& p, std::string& msg)
{
    p = ViewPlan();
    if (s < 1) return wg_plan_refuse(msg, "view: the interval starts at site %lld (sites count from 1)", (long long)s);
    if (e <= s) return wg_plan_refuse(msg, "view: the interval [%lld, %lld) is empty", (long long)s, (long long)e);
    if (e > 0x7fffffffLL) return wg_plan_refuse(msg, "view: the interval ends at site %lld (at most %lld)", (long long)e, 0x7fffffffLL);
    if (flags & ~WG_VIEW_FLAGS_ALL) return wg_plan_refuse(msg, "view: unknown flags %d", (int)flags);
    if (min_len < 1) return wg_plan_refuse(msg, "view: min_len %d (at least 1)", (int)min_len);
    if (initial_records > WG_VIEW_MAX_RECORDS) return wg_plan_refuse(msg, "view: %lld initial records (below 2^31)", (long long)initial_records);
    p.s = s; p.e = e; p.flags = flags; p.min_len = min_len;
    p.initial_records = initial_records <= 0 ? WG_VIEW_DEFAULT_RECORDS : initial_records;
    return WGBSSEG_OK;
}

// the records a chunk of n_bytes can add at most
inline int64_t wg_view_chunk_records(int64_t n_bytes) { return n_bytes / WG_VIEW_MIN_LINE + 1; }

// The growth rule of both buffers: room for `need` units where `cap` are there -> the new capacity: `cap` when it is enough, else
// at least twice as much (geometric: k growths hold 2^k times the first size).  The engine copies what the old buffer held.
inline int64_t wg_view_grow(int64_t cap, int64_t need) { return need <= cap ? cap : std::max(need, 2 * cap); }

// the records of the chunks so far + a chunk of n_bytes: refused at 2^31
inline int plan_view_chunk(int64_t n_records, int64_t n_bytes, std::string& msg)
{
    if (n_bytes > WG_VIEW_MAX_CHUNK) return wg_plan_refuse(msg, "view: a chunk of %lld bytes (at most %lld)", (long long)n_bytes, WG_VIEW_MAX_CHUNK);
    if (n_records + wg_view_chunk_records(n_bytes) > WG_VIEW_MAX_RECORDS) {
        (void)wg_plan_refuse(msg, "view: more than %lld reads selected", WG_VIEW_MAX_RECORDS);
        return WGBSSEG_E_CAPACITY;
    }
    return WGBSSEG_OK;
}

// The sort of n records: runs of WG_VIEW_RUN indices sorted in LDS, then merge passes that double the run length until one run is left.
inline int64_t wg_view_runs(int64_t n) { return (n + WG_VIEW_RUN - 1) / WG_VIEW_RUN; }
inline int wg_view_merge_passes(int64_t n)
{
    int passes = 0;
    for (int64_t runs = wg_view_runs(n); runs > 1; runs = (runs + 1) / 2) passes++;
    return passes;
}

// The files of a view over several (wgbsseg_patview_next_file): a host table of the boundaries.  end_bytes[k] / end_recs[k]: the bytes fed /
// the records kept when file k ended, counted over all files — the kernels keep their global byte offsets, and locate() turns one into
// (file, offset inside it) for a message.  The last file has no entry: it is open until finish().
struct ViewFiles {
    std::vector<int64_t> end_bytes, end_recs;
    bool several() const { return !end_bytes.empty(); }
    int64_t open_file() const { return (int64_t)end_bytes.size(); }      // the 0-based index of the file being fed
    void close(int64_t bytes, int64_t recs) { end_bytes.push_back(bytes); end_recs.push_back(recs); }
    // a file that ends at `bytes` holds the offsets below it: an offset belongs to the first file whose end lies beyond it
    void locate(uint64_t off, int64_t& file, uint64_t& inside) const
    {
        file = (int64_t)(std::upper_bound(end_bytes.begin(), end_bytes.end(), (int64_t)off) - end_bytes.begin());
        inside = off - (file ? (uint64_t)end_bytes[(size_t)file - 1] : 0u);
    }
};

// next_file(): `left` BGZF bytes that the last feed_bgzf did not take are the beginning of a member the file does not finish
inline int plan_view_next_file(bool finished, int64_t left, int64_t file, std::string& msg)
{
    if (finished) { (void)wg_plan_refuse(msg, "patview_next_file: finish() has been called"); return WGBSSEG_E_STATE; }
    if (left > 0) return wg_plan_refuse(msg, "failed in view: file %lld: truncated (%lld bytes behind its last whole BGZF member)", (long long)file, (long long)left);
    return WGBSSEG_OK;
}

// The labels of `wgbstools mix_pat` (wgbsseg_patview_set_labels): at most WG_VIEW_MAX_LABELS, distinct, each non-empty and of printable
// ASCII without white space, '/', '&' and '\' (a label goes through the reference's `sed 's/$/\tLABEL/'` untouched only without them).
// rank[k]: the place of label k in byte order, a prefix first — the order `sort` gives lines that differ in their label only; bytes /
// off: the labels in that order, one after the other, and their n + 1 offsets, as the device takes them.
struct ViewLabels {
    std::vector<uint32_t> rank, off;                                // rank: one per label as given | off: n + 1 offsets into bytes, by rank
    std::string bytes;
    int64_t n() const { return (int64_t)rank.size(); }
};

inline int plan_view_labels(const char* const* labels, int64_t n, int flags, ViewLabels& p, std::string& msg)
{
    p = ViewLabels();
    if (n < 1 || n > WG_VIEW_MAX_LABELS || !labels) return wg_plan_refuse(msg, "view: %lld labels (1 to %d)", (long long)n, WG_VIEW_MAX_LABELS);
    if (!(flags & WG_VIEW_SORT)) return wg_plan_refuse(msg, "view: labels need a sorted view (WGBSSEG_VIEW_SORT): the order of tied lines is defined on it");
    std::vector<std::string> names;
    for (int64_t k = 0; k < n; k++) {
        if (!labels[k] || !labels[k][0]) return wg_plan_refuse(msg, "view: label %lld is empty", (long long)k);
        names.emplace_back(labels[k]);
        for (const char c : names.back())
            if (c <= ' ' || c > '~' || c == '/' || c == '&' || c == '\\')
                return wg_plan_refuse(msg, "view: label %lld holds the byte 0x%02x (printable ASCII without white space, '/', '&' and '\\')", (long long)k, (unsigned)(unsigned char)c);
    }
    std::vector<uint32_t> order((size_t)n);
    for (uint32_t k = 0; k < (uint32_t)n; k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });      // (std::string: bytes as unsigned char, a prefix first)
    for (int64_t k = 1; k < n; k++)
        if (names[order[(size_t)k]] == names[order[(size_t)k - 1]]) return wg_plan_refuse(msg, "view: the label %s is given twice", names[order[(size_t)k]].c_str());
    p.rank.resize((size_t)n);
    p.off.push_back(0u);
    for (uint32_t r = 0; r < (uint32_t)n; r++) {
        p.rank[order[r]] = r;
        p.bytes += names[order[r]];
        p.off.push_back((uint32_t)p.bytes.size());
    }
    return WGBSSEG_OK;
}

// the source of a file (wgbsseg_patview_set_source): the rank of its label, T = floor(p * 2^32) with p <= 0.25, reps >= 1
inline int plan_view_source(int64_t label_rank, uint64_t T, int64_t reps, uint64_t stream, int64_t n_labels, std::string& msg)
{
    if (label_rank < 0 || label_rank >= n_labels) return wg_plan_refuse(msg, "view: label rank %lld of %lld labels", (long long)label_rank, (long long)n_labels);
    if (T > WG_VIEW_MAX_T) return wg_plan_refuse(msg, "view: T = %llu (at most 2^30: a rate of 0.25)", (unsigned long long)T);
    if (reps < 1 || reps > WG_VIEW_MAX_DRAWS) return wg_plan_refuse(msg, "view: reps = %lld (1 to 2^20)", (long long)reps);
    if (stream > 0xffffffffULL) return wg_plan_refuse(msg, "view: stream %llu (below 2^32)", (unsigned long long)stream);
    return WGBSSEG_OK;
}

// What finish() says of a refused line once next_file() has been called: the file (0-based, in feed order) and the byte offset inside it.
enum class ViewRefusal { bad_line, unsorted, low_count };
inline std::string wg_view_file_refusal(const ViewFiles& files, ViewRefusal why, uint64_t off)
{
    int64_t file = 0;
    uint64_t inside = 0;
    files.locate(off, file, inside);
    char buf[320];
    if (why == ViewRefusal::bad_line)
        snprintf(buf, sizeof buf, "failed in view: file %lld: invalid line at byte offset %llu of the file (too few columns, a site / count that is not a number, an empty pattern, or something between the count and the end of the line)", (long long)file, (unsigned long long)inside);
    else if (why == ViewRefusal::unsorted)
        snprintf(buf, sizeof buf, "failed in view: file %lld: the pat file is not sorted: the read at byte offset %llu of the file starts before the read before it", (long long)file, (unsigned long long)inside);
    else
        snprintf(buf, sizeof buf, "failed in view: file %lld: count < 1 at byte %llu", (long long)file, (unsigned long long)inside);
    return buf;
}

// a line whose count * reps is above WG_VIEW_MAX_DRAWS: "failed in view: [file K: ]count * reps above 2^20 at byte N"
inline std::string wg_view_over_refusal(const ViewFiles& files, uint64_t off)
{
    int64_t file = 0;
    uint64_t inside = off;
    char buf[128];
    if (files.several()) {
        files.locate(off, file, inside);
        snprintf(buf, sizeof buf, "failed in view: file %lld: count * reps above 2^20 at byte %llu", (long long)file, (unsigned long long)inside);
    } else
        snprintf(buf, sizeof buf, "failed in view: count * reps above 2^20 at byte %llu", (unsigned long long)inside);
    return buf;
}

// the fetch of [offset, offset + len) in slabs of WG_VIEW_SLAB bytes: how many, and slab k's bytes
inline int64_t wg_view_slabs(int64_t len) { return (len + WG_VIEW_SLAB - 1) / WG_VIEW_SLAB; }
inline int64_t wg_view_slab_len(int64_t len, int64_t k) { return std::min<int64_t>(WG_VIEW_SLAB, len - k * WG_VIEW_SLAB); }

inline int plan_view_read(int64_t offset, int64_t len, int64_t total, const void* buf, std::string& msg)
{
    if (offset < 0 || len < 0 || offset + len > total || (len && !buf))
        return wg_plan_refuse(msg, "view: read of [%lld, %lld) from %lld bytes of output", (long long)offset, (long long)(offset + len), (long long)total);
    return WGBSSEG_OK;
}
