// tests/native/san_bed2beta.cpp — a stand-alone program over wgbs_tools_amd/csrc/bed2beta_plan.h and bed2beta_core.h for the sanitizers
// (tests/test_bed2beta_cpu.py builds it plain and with -fsanitize=address,undefined and runs it directly): the whole of `bed2beta` on the
// host by the functions the kernels call (bed2beta_run.h) — plan the chromosome table, walk every line, find its chromosome and its CpG,
// lower the site's word, unpack.  The text, the loci, the table and the result are heap arrays of exactly their size, so a byte read or
// written beyond one is seen.
//   san_bed2beta BED LOCI CHROMS flags     (LOCI: uint32 binary; CHROMS: lines "name\tCpGs"; flags: 1 ADD_ONE, 2 HEADER)
//   -> the .beta bytes on stdout; "stats a b c d e f" or the refusal on stderr (exit 4)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "bed2beta_run.h"

static char* slurp(const char* path, size_t& n)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return nullptr; }
    fseek(f, 0, SEEK_END);
    n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    char* p = static_cast<char*>(malloc(n ? n : 1));
    if (n && fread(p, 1, n, f) != n) { fclose(f); free(p); return nullptr; }
    fclose(f);
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: san_bed2beta BED LOCI CHROMS flags\n"); return 2; }
    size_t nt = 0, nl = 0, nc = 0;
    char* text = slurp(argv[1], nt);
    char* loci_raw = slurp(argv[2], nl);
    char* table = slurp(argv[3], nc);
    if (!text || !loci_raw || !table) return 2;
    const uint32_t* loci = reinterpret_cast<const uint32_t*>(loci_raw);
    const int64_t n_sites = (int64_t)(nl / 4);
    std::vector<std::string> names;
    std::vector<int64_t> lo, hi;
    int64_t at = 0;
    for (size_t p = 0; p < nc;) {
        size_t e = p;
        while (e < nc && table[e] != '\n') e++;
        const char* tab = static_cast<const char*>(memchr(table + p, '\t', e - p));
        if (tab) {
            names.emplace_back(table + p, (size_t)(tab - (table + p)));
            const int64_t size = atoll(std::string(tab + 1, (size_t)(table + e - tab - 1)).c_str());
            lo.push_back(at); hi.push_back(at + size);
            at += size;
        }
        p = e + 1;
    }
    std::vector<const char*> ptr;
    for (const auto& s : names) ptr.push_back(s.c_str());
    const int32_t flags = atoi(argv[4]);
    BedBetaPlan plan;
    std::string msg;
    if (plan_bedbeta(loci, n_sites, ptr.data(), lo.data(), hi.data(), (int32_t)ptr.size(), flags, plan, msg) != WGBSSEG_OK) { fprintf(stderr, "%s\n", msg.c_str()); return 3; }
    uint8_t* out = static_cast<uint8_t*>(malloc((size_t)n_sites * 2));
    int64_t stats[6];
    unsigned long long report = ~0ULL;
    bb_run_host(text, (int64_t)nt, plan, loci, flags, out, stats, &report);
    int rc = 0;
    if (wg_bb_refusal(report, msg)) { fprintf(stderr, "%s\n", msg.c_str()); rc = 4; }
    else {
        fwrite(out, 1, (size_t)n_sites * 2, stdout);
        fprintf(stderr, "stats %lld %lld %lld %lld %lld %lld\n", (long long)stats[0], (long long)stats[1], (long long)stats[2], (long long)stats[3], (long long)stats[4], (long long)stats[5]);
    }
    free(out); free(table); free(loci_raw); free(text);
    return rc;
}
