// tests/native/san_fasta.cpp — a stand-alone program over wgbs_tools_amd/csrc/fasta_core.h and fasta_plan.h for the sanitizers
// (tests/test_init_genome_cpu.py builds it plain and with -fsanitize=address,undefined and runs it directly).  It does what the engine
// does, on the host: the text is cut into chunks at the given offsets; per chunk the pending C is settled, every 16-byte stretch is
// counted for each of the four entry states (wg_fa_count) and the stretches are composed left to right (wg_fa_map_then, wg_fa_sum_then,
// wg_fa_cur_then) from the carry, as k_fa_measure and k_fa_scan compose them; then every stretch is walked from where the composition says
// the walk stands (wg_fa_walk), as k_fa_pack walks it.  The text is a heap array of exactly its size, every chunk a copy of exactly its
// size, so a look ahead beyond one is seen.  The result must equal one serial walk over the whole text: exit status 4 says it does not.
//   san_fasta FASTA [cut ...]   -> per sequence "name \t offset \t bases \t sites", then "loci" and the loci, then "refused" and the word
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "fasta_plan.h"

struct Text {
    const char* p;
    char at(int64_t i) const { return p[i]; }
};

struct Found {
    std::vector<wg_fa_seq> seqs;
    std::map<uint64_t, uint32_t> loci;                             // by place: the order of arrival is not FASTA order in pieces
    uint64_t bad = ~0ULL;
    bool pend = false;
    uint64_t pend_locus = 0;
    wg_fa_seq& rec(uint64_t i)
    {
        if (seqs.size() <= i) seqs.resize(i + 1, wg_fa_seq{});
        return seqs[i];
    }
    void header(const wg_fa_cur& c, uint64_t at) { wg_fa_seq& r = rec(c.seqs); r.hdr_off = at; r.first_locus = c.hits; r.prev_bases = (uint32_t)c.bases; }
    void name_byte(uint64_t seq, uint32_t idx, char b) { rec(seq).name[idx] = b; }
    void name_end(uint64_t seq, uint64_t len) { rec(seq).name_len = (uint32_t)std::min<uint64_t>(len, WG_FA_MAX_NAME + 1); }
    void hit(uint64_t index, uint64_t locus) { loci[index] = (uint32_t)locus; }
    void pending(uint64_t locus) { pend = true; pend_locus = locus; }
    void refuse(uint64_t at, int why) { bad = std::min<uint64_t>(bad, (at << 8) | (uint64_t)why); }
};

static void close_last(Found& f, const wg_fa_cur& c, uint64_t n)
{
    if (c.seqs && c.state == WG_FA_NM) {
        const uint64_t len = n - c.hdr_off - 1;
        if (len == 0) f.refuse(c.hdr_off, WG_FA_BAD_EMPTY_NAME);
        f.rec(c.seqs - 1).name_len = (uint32_t)std::min<uint64_t>(len, WG_FA_MAX_NAME + 1);
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: san_fasta FASTA [cut ...]\n"); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    fseek(fh, 0, SEEK_END);
    const int64_t n = (int64_t)ftell(fh);
    fseek(fh, 0, SEEK_SET);
    char* whole = static_cast<char*>(malloc(n ? (size_t)n : 1));
    if (n && fread(whole, 1, (size_t)n, fh) != (size_t)n) return 2;
    fclose(fh);
    std::vector<int64_t> cuts = {0};
    for (int k = 2; k < argc; k++) cuts.push_back(std::min<int64_t>(std::max<int64_t>(atoll(argv[k]), cuts.back()), n));
    cuts.push_back(n);

    // one serial walk
    Found serial;
    wg_fa_cur sc = {0, 0, 0, 0, WG_FA_LS};
    { const Text T = {whole}; wg_fa_walk(T, n, 0, n, 0, sc, serial); }
    close_last(serial, sc, (uint64_t)n);

    // the engine's way
    Found tiled;
    wg_fa_cur carry = {0, 0, 0, 0, WG_FA_LS};
    for (size_t k = 0; k + 1 < cuts.size(); k++) {
        const int64_t a = cuts[k], m = cuts[k + 1] - a;
        if (m == 0) continue;
        char* chunk = static_cast<char*>(malloc((size_t)m));
        memcpy(chunk, whole + a, (size_t)m);
        const Text T = {chunk};
        if (tiled.pend) {                                           // k_fa_settle
            const int g = wg_fa_next_is_g(T, m, 0, carry.state == WG_FA_LS);
            if (g > 0) { tiled.loci[carry.hits] = (uint32_t)tiled.pend_locus; carry.hits++; }
            if (g >= 0) tiled.pend = false;
        }
        wg_fa_cur c = carry;
        for (int64_t p0 = 0; p0 < m; p0 += WG_FA_THREAD_BYTES) {
            const int64_t p1 = std::min<int64_t>(p0 + WG_FA_THREAD_BYTES, m);
            uint32_t map = 0;
            wg_fa_sum sums[4];
            for (uint32_t s = 0; s < 4; s++) {                      // k_fa_measure: every entry state
                uint32_t leaves = s;
                sums[s] = wg_fa_count(T, m, p0, p1, 0, s, &leaves);
                map |= leaves << (2 * s);
            }
            wg_fa_cur w = c;                                        // k_fa_pack: from where the composition stands
            wg_fa_walk(T, m, p0, p1, (uint64_t)a, w, tiled);
            const wg_fa_sum& s = sums[c.state];                     // k_fa_scan: the composition goes on
            wg_fa_cur_then(c, wg_fa_sum64{s.h, s.pre, s.post, s.hits, (uint64_t)a + s.last});
            c.state = wg_fa_map_at(wg_fa_map_then(WG_FA_MAP_ID, map), c.state);
            if (w.seqs != c.seqs || w.bases != c.bases || w.hits != c.hits || w.state != c.state || (c.seqs && w.hdr_off != c.hdr_off)) {
                fprintf(stderr, "the composition and the walk part at byte %lld\n", (long long)(a + p1));
                return 4;
            }
        }
        carry = c;
        free(chunk);
    }
    close_last(tiled, carry, (uint64_t)n);

    bool same = serial.seqs.size() == tiled.seqs.size() && serial.loci == tiled.loci && serial.bad == tiled.bad && sc.seqs == carry.seqs && sc.hits == carry.hits &&
                sc.bases == carry.bases && sc.state == carry.state;
    for (size_t i = 0; same && i < serial.seqs.size(); i++) {
        const wg_fa_seq &x = serial.seqs[i], &y = tiled.seqs[i];
        same = x.hdr_off == y.hdr_off && x.first_locus == y.first_locus && x.prev_bases == y.prev_bases && x.name_len == y.name_len &&
               memcmp(x.name, y.name, std::min<uint32_t>(x.name_len, WG_FA_MAX_NAME)) == 0;
    }
    if (!same) { fprintf(stderr, "the chunks and the serial walk differ\n"); return 4; }
    std::string msg;
    if (serial.bad == ~0ULL && plan_fasta_names(serial.seqs, msg) != WGBSSEG_OK) { printf("%s\n", msg.c_str()); free(whole); return 0; }
    for (size_t i = 0; i < tiled.seqs.size(); i++) {
        const wg_fa_seq& r = tiled.seqs[i];
        const uint64_t bases = i + 1 < tiled.seqs.size() ? tiled.seqs[i + 1].prev_bases : carry.bases;
        const uint64_t sites = (i + 1 < tiled.seqs.size() ? tiled.seqs[i + 1].first_locus : carry.hits) - r.first_locus;
        printf("%.*s\t%llu\t%llu\t%llu\n", (int)std::min<uint32_t>(r.name_len, WG_FA_MAX_NAME), r.name, (unsigned long long)r.hdr_off, (unsigned long long)bases, (unsigned long long)sites);
    }
    printf("loci");
    for (const auto& kv : tiled.loci) printf(" %u", kv.second);
    printf("\nrefused %llu\n", (unsigned long long)tiled.bad);
    if (tiled.bad != ~0ULL) { (void)wg_fa_refuse(msg, tiled.bad); printf("%s\n", msg.c_str()); }
    free(whole);
    return 0;
}
