// Host check of csrc/lr_schedule.h: the text the one-workgroup kernel of lr_schedule.hip runs, called here over a case file and printed
// as bits, so that a test can compare them with Python's own arithmetic (tests/test_lr_scheduler.py) - same libm, same operation
// order.  A stand-alone program with its own main; build it with
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I vit-ed_amd/csrc
// Every table lives in an exactly-sized heap buffer, so a read past the last milestone word is reported.
//
// Input (argv[1]), one case per line:   LRS_TABLE_WORDS table words, base, scale   as 16-digit hex bit patterns, then t in decimal
// Output, one line per case:            bits of lr_schedule_value(table, base, t)   bits of (float)(value * scale)
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <memory>

#include "lr_schedule.h"

static double from_bits(uint64_t u) {
    double d;
    memcpy(&d, &u, 8);
    return d;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    long cases = 0;
    for (;;) {
        std::unique_ptr<double[]> table(new double[LRS_TABLE_WORDS]);
        uint64_t u = 0;
        int got = 0;
        for (; got < LRS_TABLE_WORDS && fscanf(f, "%" SCNx64, &u) == 1; ++got) table[got] = from_bits(u);
        if (got == 0) break;
        uint64_t base_bits = 0, scale_bits = 0;
        int64_t t = 0;
        if (got != LRS_TABLE_WORDS || fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNd64, &base_bits, &scale_bits, &t) != 3) {
            fprintf(stderr, "case %ld is incomplete\n", cases);
            return 1;
        }
        const double v = lr_schedule_value(table.get(), from_bits(base_bits), t);
        const float lr = (float)(v * from_bits(scale_bits));
        uint64_t vb;
        uint32_t lb;
        memcpy(&vb, &v, 8);
        memcpy(&lb, &lr, 4);
        printf("%016" PRIx64 " %08" PRIx32 "\n", vb, lb);
        ++cases;
    }
    fclose(f);
    printf("lrsched_host_check ok: %ld cases\n", cases);
    return 0;
}
