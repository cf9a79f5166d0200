// tests/host/stitch_thresholds.cpp -- TEST TOOL, never shipped or loaded by the product.
//
// Prints the table that carries read stitching's one float32 decision (mm / sl > x) into the kernels' integers: the very
// mkt::stitch_thresholds of microcket_amd/csrc/mkt_stitch.h, so that tests/test_stitch_edges_host.py can hold it against float32
// arithmetic done in numpy, without a GPU.
//
//   stitch_thresholds M x [M x ...]     one line per (M, x): thr[1] ... thr[255]
//   stitch_thresholds                   the same for "M x" lines read from stdin
// x is read as a double and cast to float, as mkt_stitch_begin does with its argument.
#include <cstdio>
#include <cstdlib>
#include "../../microcket_amd/csrc/mkt_stitch.h"

static int one(const char* sM, const char* sx) {
    char *e1 = nullptr, *e2 = nullptr;
    const unsigned long M = strtoul(sM, &e1, 10);
    const double x = strtod(sx, &e2);
    char msg[256];
    if (e1 == sM || *e1 || e2 == sx || *e2 || mkt::stitch_check_args(M < 1 ? 1u : (uint32_t)M, (uint32_t)M, x, 33, 10, 36, msg, sizeof msg) != MKT_OK) {
        fprintf(stderr, "bad (M, x): %s %s\n", sM, sx);
        return 2;
    }
    uint16_t thr[MKT_STITCH_MAX_M + 1];
    mkt::stitch_thresholds((uint32_t)M, (float)x, thr);
    for (int sl = 1; sl <= MKT_STITCH_MAX_M; ++sl) printf("%u%c", (unsigned)thr[sl], sl < MKT_STITCH_MAX_M ? ' ' : '\n');
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        if ((argc - 1) % 2) { fprintf(stderr, "usage: %s M x [M x ...]   (or \"M x\" lines on stdin)\n", argv[0]); return 2; }
        for (int k = 1; k < argc; k += 2) if (int rc = one(argv[k], argv[k + 1])) return rc;
        return 0;
    }
    char a[64], b[64];
    while (scanf("%63s %63s", a, b) == 2) if (int rc = one(a, b)) return rc;
    return 0;
}
