// Host-only check of the pure parts of genarchbench_amd/csrc/gab_pair_stage.h (the window scan and the staging layout; no HIP
// call), meant to run under the host sanitizers:
//   hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all -o pair_stage_check tools/pair_stage_check.cpp
// stdin: per case a line "<name> <1 if pat and txt are one slab> <n>" and n lines "<pat_off> <pat_len> <txt_off> <txt_len>".
// stdout: per case the window, then the offsets of every array of the three layouts.  Exit status 1 when a window differs from the
// plain min / max over the pairs, an 8-byte array is not 8-byte aligned, the cursor is not 256-byte aligned or the layout is too small.
#include "../genarchbench_amd/csrc/gab_pair_stage.h"
#include <string>
#include <vector>

void gab_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); }

int main() {
    char name[128]; int same = 0, bad = 0; long long n = 0;
    while (scanf("%127s %d %lld", name, &same, &n) == 3) {
        std::vector<int64_t> po(n), to(n); std::vector<int32_t> pl(n), tl(n);
        int64_t lo[2] = {INT64_MAX, INT64_MAX}, hi[2] = {0, 0}, ops = 0;
        for (long long i = 0; i < n; i++) {
            long long a, b, c, d;
            if (scanf("%lld %lld %lld %lld", &a, &b, &c, &d) != 4) return 2;
            po[i] = a; pl[i] = (int32_t)b; to[i] = c; tl[i] = (int32_t)d; ops += b + d;
            lo[0] = std::min<int64_t>(lo[0], a); hi[0] = std::max<int64_t>(hi[0], a + b);
            lo[1] = std::min<int64_t>(lo[1], c); hi[1] = std::max<int64_t>(hi[1], c + d);
        }
        const char *slab = (const char *)0x10000;              // (never dereferenced: the scan compares the two pointers)
        const gab_host_pairs in = {slab, po.data(), pl.data(), same ? slab : slab + 1, to.data(), tl.data(), n};
        gab_pair_window w;
        if (gab_pair_scan(name, in, &w) != GAB_OK) { printf("%s rejected\n", name); continue; }
        printf("%s pa %lld pb %lld ta %lld tb %lld shared %d ppad %zu tpad %zu\n", name, (long long)w.pa, (long long)w.pb, (long long)w.ta,
               (long long)w.tb, (int)w.shared, w.ppad, w.tpad);
        // every pair inside its window, the window no wider than the 256 bytes the start rounds down by, room for a dword read at the end
        bad += w.pa > lo[0] || w.pb < hi[0] || w.ta > lo[1] || w.tb < hi[1] || w.pa % 256 || w.ta % 256;
        if (!w.shared) bad += lo[0] - w.pa > 255 || w.pb != hi[0] || lo[1] - w.ta > 255 || w.tb != hi[1] || w.tpad < (size_t)(w.tb - w.ta) + 3;
        else bad += !same || w.pa != w.ta || w.pb != w.tb || std::min(lo[0], lo[1]) - w.pa > 255 || w.pb != std::max(hi[0], hi[1]) || w.tpad != 0;
        bad += w.ppad < (size_t)(w.pb - w.pa) + 3 || w.ppad % 256 || w.tpad % 256;
        for (int kind = GAB_STAGE_SCORES; kind <= GAB_STAGE_TEXT; kind++) {
            const size_t nn = (size_t)n, opad = gab_pad256((size_t)ops + 16), cpad = gab_pad256((size_t)ops / 4 + 4096);
            const gab_pair_layout L = gab_pair_layout_of((gab_pair_stage_kind)kind, w.ppad, w.tpad, nn, opad, cpad);
            printf("  kind %d: p %zu t %zu ops %zu text %zu | po %zu to %zu oo %zu co %zu | pl %zu tl %zu ol %zu cl %zu sc %zu | cur %zu | bytes %zu\n", kind,
                   L.p, L.t, L.ops, L.text, L.po, L.to, L.oo, L.co, L.pl, L.tl, L.ol, L.cl, L.sc, L.cur, L.bytes);
            bad += L.po % 8 || L.to % 8 || L.oo % 8 || L.co % 8 || L.cur % 256 || L.p % 256 || L.t % 256 || L.ops % 256 || L.text % 256;
            bad += L.t < L.p + w.ppad || L.po < L.t + w.tpad || L.bytes < L.sc + 4 * nn || (kind == GAB_STAGE_TEXT && L.bytes < L.cur + 8);
        }
    }
    if (bad) fprintf(stderr, "pair_stage_check: %d check(s) failed\n", bad);
    return bad != 0;
}
