// tests/native/san_bam2pat.cpp — a stand-alone program over wgbs_tools_amd/csrc/sam_plan.h and sam_core.h for the sanitizers
// (tests/test_bam2pat_cpu.py builds it plain and with -fsanitize=address,undefined and runs it directly): the whole of `bam2pat` on the
// host by the functions the kernels call (sam_run.h) — plan the chromosome table, read every line, walk its CIGAR and the loci under it,
// find the mates, merge, sort and count.  The text, the loci and the table are heap arrays of exactly their size, so a byte read beyond
// one is seen.
//   san_bam2pat SAM LOCI CHROMS paired exclude include mapq strand clip min_cpg     (LOCI: uint32 binary; CHROMS: lines "name\tCpGs")
//   -> the pat text on stdout; "stats" and the ten counters on stderr
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "sam_run.h"

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
    if (argc != 11) { fprintf(stderr, "usage: san_bam2pat SAM LOCI CHROMS paired exclude include mapq strand clip min_cpg\n"); return 2; }
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
    SamPlan plan;
    std::string msg;
    if (plan_sam(loci, n_sites, ptr.data(), lo.data(), hi.data(), (int32_t)ptr.size(), atoi(argv[4]), atoll(argv[5]), atoll(argv[6]), atoi(argv[7]), atoi(argv[8]), atoi(argv[9]),
                 atoi(argv[10]), plan, msg) != WGBSSEG_OK) {
        fprintf(stderr, "%s\n", msg.c_str());
        return 3;
    }
    int64_t stats[WG_SAM_COUNTERS];
    const std::string out = sam_run_host(text, (int64_t)nt, plan, loci, stats);
    fwrite(out.data(), 1, out.size(), stdout);
    fprintf(stderr, "stats");
    for (int k = 0; k < WG_SAM_COUNTERS; k++) fprintf(stderr, " %lld", (long long)stats[k]);
    fprintf(stderr, "\n");
    free(table); free(loci_raw); free(text);
    return 0;
}
