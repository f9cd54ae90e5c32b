// fasta_plan.h — the host plan of `wgbstools init_genome`'s engine (wgbsseg_fasta): the shapes of its launches, the BGZF plan WITHOUT
// the line rule (a chunk of FASTA text may be cut at any byte: an unwrapped chromosome is one line of 250 MB), the messages of the
// refusals, the checks of select() and the bound on a dictionary line.  No HIP here (like view_plan.h): g++ compiles it alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "inflate_plan.h"
#include "view_plan.h"
#include "fasta_core.h"

#define WG_FA_TILE 4096                // bytes of text one workgroup of k_fa_measure / k_fa_pack reads
#define WG_FA_BLOCK 256                // its threads
#define WG_FA_THREAD_BYTES 16          // ... and the bytes of each
#define WG_FA_SCAN_BLOCK 256           // threads of k_fa_scan's one workgroup; each takes a run of consecutive tiles
#define WG_FA_MAX_CHUNK 0x7fffffffLL   // bytes of one chunk
#define WG_FA_INITIAL_SEQS 64
#define WG_FA_INITIAL_LOCI (1 << 20)
#define WG_FA_DICT_BLOCK 256           // sites (= threads) of one workgroup of k_dict_len / k_dict_emit
#define WG_FA_DICT_TAIL 23             // "\t4294967295\t4294967295\n"
#define WG_FA_DICT_MAX_LINE (WG_FA_MAX_NAME + WG_FA_DICT_TAIL)
#define WG_FA_DICT_STAGE 16384         // bytes of LDS a workgroup of k_dict_emit formats its lines in, when they fit
#define WG_FA_MAX_SITES 0xffffffffLL   // a site number is printed from 32 bits
static_assert(WG_FA_TILE == WG_FA_BLOCK * WG_FA_THREAD_BYTES, "a thread per 16 bytes of a tile");
static_assert(WG_FA_DICT_BLOCK * 48 <= WG_FA_DICT_STAGE, "the lines of any genome whose names have 25 bytes are staged");

inline int64_t wg_fa_tiles(int64_t n_bytes) { return (n_bytes + WG_FA_TILE - 1) / WG_FA_TILE; }
inline int64_t wg_fa_tiles_per_thread(int64_t tiles) { return (tiles + WG_FA_SCAN_BLOCK - 1) / WG_FA_SCAN_BLOCK; }

inline const char* wg_fa_what(int reason)
{
    static const char* const what[WG_FA_BAD_REASONS] = {
        "no error", "text before the first header line", "a header line with an empty name", "a sequence name of more than 255 bytes",
        "a byte in a sequence that is not printable ASCII (0x21 .. 0x7E)", "a sequence of more than 4294967294 bases"};
    return reason > 0 && reason < WG_FA_BAD_REASONS ? what[reason] : "unknown error";
}

// "Invalid FASTA: <what> at byte offset N of the text"
inline int wg_fa_refuse(std::string& msg, uint64_t word)
{
    return wg_plan_refuse(msg, "Invalid FASTA: %s at byte offset %llu of the text", wg_fa_what((int)(word & 0xff)), (unsigned long long)(word >> 8));
}

inline int plan_fasta_chunk(int64_t n_bytes, std::string& msg)
{
    if (n_bytes > WG_FA_MAX_CHUNK) return wg_plan_refuse(msg, "fasta: a chunk of %lld bytes (at most %lld)", (long long)n_bytes, WG_FA_MAX_CHUNK);
    return WGBSSEG_OK;
}

// The complete members of bytes[0 .. n), all for the device, their text from the front of the text buffer: no carry, no line rule
// (BgzfPlan as PatFeed::stage_bgzf reads it)
inline int plan_bgzf_bytes(const uint8_t* bytes, int64_t n, uint64_t file_base, BgzfPlan& p, std::string& msg)
{
    p = BgzfPlan();
    const int rc = bgzf_walk(bytes, n, file_base, p.members, &p.consumed, msg);
    if (rc != WGBSSEG_OK) return rc;
    p.n_dev = (int64_t)p.members.size();
    if (p.n_dev) {
        const wg_bgzf_member& last = p.members.back();
        p.comp_bytes = (int64_t)(last.in_off + last.in_len + 8);
        p.text_cap = p.n_text = (int64_t)(last.out_off + last.isize);
    }
    return WGBSSEG_OK;
}

// select(): the kept sequences in dictionary order, each once
inline int plan_fasta_select(const int64_t* order, int64_t n_order, int64_t n_seqs, const std::vector<int64_t>& n_sites, int64_t* total, std::string& msg)
{
    *total = 0;
    if (n_order < 0 || (n_order && !order)) return wg_plan_refuse(msg, "bad arguments to fasta_select");
    if (n_order == 0) return wg_plan_refuse(msg, "Invalid FASTA: no chromosome is kept (none of the %lld sequence names is chr1, 1, chrX, MT, ...)", (long long)n_seqs);
    std::vector<char> seen((size_t)n_seqs, 0);
    for (int64_t k = 0; k < n_order; k++) {
        const int64_t i = order[k];
        if (i < 0 || i >= n_seqs) return wg_plan_refuse(msg, "fasta_select: sequence %lld of %lld", (long long)i, (long long)n_seqs);
        if (seen[(size_t)i]) return wg_plan_refuse(msg, "fasta_select: sequence %lld is selected twice", (long long)i);
        seen[(size_t)i] = 1;
        *total += n_sites[(size_t)i];
    }
    if (*total > WG_FA_MAX_SITES) return wg_plan_refuse(msg, "fasta_select: %lld sites (at most %lld)", (long long)*total, WG_FA_MAX_SITES);
    return WGBSSEG_OK;
}

// finish_scan(): two sequences with one name (names: the table come home) -> the message
inline int plan_fasta_names(const std::vector<wg_fa_seq>& seqs, std::string& msg)
{
    std::vector<size_t> idx(seqs.size());
    for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
    const auto name = [&](size_t i) { return std::string(seqs[i].name, seqs[i].name_len); };
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { const std::string x = name(a), y = name(b); return x != y ? x < y : a < b; });
    uint64_t first = ~0ULL;
    size_t which = 0;
    for (size_t k = 1; k < idx.size(); k++)
        if (name(idx[k]) == name(idx[k - 1]) && seqs[idx[k]].hdr_off < first) { first = seqs[idx[k]].hdr_off; which = idx[k]; }
    if (first == ~0ULL) return WGBSSEG_OK;
    return wg_plan_refuse(msg, "Invalid FASTA: the sequence name %s of the header at byte offset %llu of the text has been used before", name(which).c_str(), (unsigned long long)first);
}
