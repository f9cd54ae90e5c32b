// Sanitizer harness for the DEFLATE encoder shared by the host and the device (TEST INFRASTRUCTURE): csrc/deflate_core.h's host twin over
// a file of texts that tests/deflate_cases.py writes — records of {u32 bytes, text}.  Every text is copied into a heap array of exactly
// its size and encoded into a heap array of exactly 18 + n + 5 + 8 bytes, so that a read or a write past either end is seen; the member is
// then inflated by csrc/inflate_core.h's host twin into an array of exactly n bytes and compared.  Prints one line per record: the
// member's size, a checksum of its bytes and whether the text came back.  tests/test_deflate_cpu.py builds it plain and with
// AddressSanitizer + UndefinedBehaviorSanitizer and compares the lines.
#include <cstdio>
#include <cstring>
#include "deflate_plan.h"
#include "inflate_core.h"

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: san_deflate texts\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    long records = 0, back = 0;
    for (;;) {
        uint32_t n;
        if (fread(&n, 4, 1, f) != 1) break;
        if (n > WG_DEF_MEMBER) { fprintf(stderr, "a text of %u bytes\n", n); return 2; }
        uint8_t* text = new uint8_t[n ? n : 1];
        if (n && fread(text, 1, n, f) != n) { fprintf(stderr, "short file\n"); return 2; }
        const size_t room = (size_t)WG_DEF_HEAD + n + 5 + WG_DEF_TAIL;
        uint8_t* member = new uint8_t[room];
        const uint32_t size = deflate_member_host(n ? text : nullptr, n, member);
        unsigned long sum = 0;
        for (uint32_t i = 0; i < size && i < room; i++) sum = sum * 31 + member[i];
        uint8_t* again = new uint8_t[n ? n : 1];
        int same = 0;
        if (size >= WG_DEF_HEAD + WG_DEF_TAIL && size <= room) {
            const int rc = inflate_member_host(member + WG_DEF_HEAD, (int64_t)size - WG_DEF_HEAD - WG_DEF_TAIL, again, n);
            same = rc == WG_INF_OK && (n == 0 || memcmp(again, text, n) == 0);
        }
        printf("%ld: %u -> %u %lu back %d\n", records, n, size, sum, same);
        records += 1;
        back += same;
        delete[] again;
        delete[] member;
        delete[] text;
    }
    fclose(f);
    printf("records: %ld, back: %ld\n", records, back);
    return 0;
}
