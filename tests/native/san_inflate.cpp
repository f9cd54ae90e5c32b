// Sanitizer harness for the DEFLATE decoder shared by the host and the device (TEST INFRASTRUCTURE): csrc/inflate_core.h's host twin
// and csrc/inflate_plan.h's member walk over a corpus file that tests/inflate_cases.py writes — records of {u32 payload bytes, u32 ISIZE,
// payload}.  Every payload is copied into a heap array of exactly its size and decoded into a heap array of exactly ISIZE bytes, so
// that a read or a write past either end is seen; each record is also wrapped as a BGZF member in an exact-size array and walked.
// Prints one line per record: the twin's code and a checksum of the text.  tests/test_inflate_cpu.py builds it plain and with
// AddressSanitizer + UndefinedBehaviorSanitizer and compares the lines.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "inflate_plan.h"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: san_inflate corpus\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    long records = 0, refused = 0;
    for (;;) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) break;
        const uint32_t n_in = hdr[0], isize = hdr[1];
        uint8_t* payload = new uint8_t[n_in ? n_in : 1];
        if (n_in && fread(payload, 1, n_in, f) != n_in) { fprintf(stderr, "short corpus\n"); return 2; }
        uint8_t* text = new uint8_t[isize ? isize : 1];
        memset(text, 0, isize ? isize : 1);
        const int rc = inflate_member_host(n_in ? payload : nullptr, n_in, text, isize);
        unsigned long sum = 0;
        if (rc == WG_INF_OK) for (uint32_t i = 0; i < isize; i++) sum = sum * 31 + text[i];
        // the same payload as a BGZF member, cut at every length that matters to the walk
        const size_t size = 18 + (size_t)n_in + 8;
        int walked = -1;
        if (size <= 65536) {
            uint8_t* mem = new uint8_t[size];
            const uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)((size - 1) & 0xff), (uint8_t)((size - 1) >> 8)};
            memcpy(mem, head, 18);
            if (n_in) memcpy(mem + 18, payload, n_in);
            memset(mem + 18 + n_in, 0, 4);
            for (int k = 0; k < 4; k++) mem[18 + n_in + 4 + k] = (uint8_t)(isize >> (8 * k));
            walked = 0;
            for (size_t cut : {(size_t)1, (size_t)11, (size_t)12, (size_t)17, (size_t)18, size - 1, size}) {
                if (cut > size) continue;
                uint8_t* part = new uint8_t[cut];
                memcpy(part, mem, cut);
                std::vector<wg_bgzf_member> members;
                std::string msg;
                int64_t consumed = -1;
                const int wrc = bgzf_walk(part, (int64_t)cut, 1000, members, &consumed, msg);
                if (wrc == WGBSSEG_OK && consumed == (int64_t)size && members.size() == 1 && members[0].in_len == n_in && members[0].isize == isize) walked += 1;
                delete[] part;
            }
            delete[] mem;
        }
        printf("%ld: %d %s %lu walked %d\n", records, rc, wg_inflate_what(rc), sum, walked);
        records += 1;
        refused += rc != WG_INF_OK;
        delete[] text;
        delete[] payload;
    }
    fclose(f);
    printf("records: %ld, refused: %ld\n", records, refused);
    return 0;
}
