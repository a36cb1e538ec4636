// wfa_plan_dump -- prints what wfa_plan.h decides, for tests/test_wfa_plan.py to hold against the model of tests/util.py.
//   wfa_plan_dump <adaptive 0|1> <x> <o> <e> <n_lds> <no_static 0|1> <pool2 | -1> <slots | -1> <length> ...
// First the score table of the penalties, one line `row score lo hi has_gap used_end` each; then, for every (max_plen, max_tlen)
// of the lengths given, `plan max_plen max_tlen`, the launches as `kernel pool dir` spelled as in the GAB_WFA_TRACE lines, and
// `vals seqp seqt static_rows static_pool use_static byte_ok slots`.
#include "wfa_plan.h"
#include <stdlib.h>

int main(int argc, char **argv) {
    if (argc < 10) { fprintf(stderr, "usage: wfa_plan_dump adaptive x o e n_lds no_static pool2 slots length...\n"); return 2; }
    const bool adaptive = atoi(argv[1]) != 0;
    const WfaTable t = wfa_table(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    const uint32_t n_lds = (uint32_t)strtoul(argv[5], nullptr, 10);
    WfaKnobs knobs;
    knobs.no_static = atoi(argv[6]) != 0; knobs.pool2 = atoi(argv[7]); knobs.slots = atoi(argv[8]);
    for (const WfRow &r : t.rows) printf("row %d %d %d %d %d\n", r.score, r.lo, r.hi, r.has_gap, r.used_end);
    for (int i = 9; i < argc; i++)
        for (int j = 9; j < argc; j++) {
            const WfaPlan p = wfa_plan(adaptive, adaptive ? 0 : (int)t.rows.size(), atoi(argv[i]), atoi(argv[j]), n_lds, knobs);
            printf("plan %s %s\n", argv[i], argv[j]);
            for (const WfaLaunch &l : p.launches) {
                char kernel[40];
                wfa_launch_name(l, kernel, sizeof kernel);
                printf("%s %lld %lld\n", kernel, l.pool, l.dir);
            }
            printf("vals %d %d %d %d %d %d %u\n", p.seqp, p.seqt, p.static_rows, p.static_pool, (int)p.use_static, (int)p.byte_ok, p.slots);
        }
    return 0;
}
