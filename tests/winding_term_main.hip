// stand-alone: the term code of csrc/tirt_winding.h on the host, on exactly-sized heap arrays: rows from a file through wn_kat_row into a file
//   winding_term_main <rows.f32> <out.u32> <is_sphere>
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tirt_winding.h"
using namespace tirt;
int main(int argc, char **argv)
{
    if (argc != 4) { printf("usage: winding_term_main rows out is_sphere\n"); return 2; }
    const int is_sphere = atoi(argv[3]), stride = is_sphere ? WN_KAT_SPH : WN_KAT_TRI;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const long n = bytes / (long)(sizeof(float) * stride);
    float *in = new float[(size_t)n * stride];               // exactly n rows: a read of row n is out of bounds
    uint32_t *out = new uint32_t[(size_t)n * WN_KAT_OUT];
    if (fread(in, sizeof(float) * stride, (size_t)n, f) != (size_t)n) { printf("FAIL: short read\n"); return 1; }
    fclose(f);
    long long total = 0;
    for (long i = 0; i < n; i++) {
        wn_kat_row(in + (size_t)i * stride, is_sphere, out + (size_t)i * WN_KAT_OUT);
        total += (long long)(((unsigned long long)out[(size_t)i * WN_KAT_OUT + 3] << 32) | out[(size_t)i * WN_KAT_OUT + 2]);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out, sizeof(uint32_t) * WN_KAT_OUT, (size_t)n, f) != (size_t)n) { printf("FAIL: cannot write %s\n", argv[2]); return 1; }
    fclose(f);
    delete[] in; delete[] out;
    printf("winding_term_main: %ld rows, the sum of their terms is %lld, w = %.9g\n", n, total, (double)wn_result(total));
    return 0;
}
