// Stand-alone check of the ICC profile reader (grok_amd/csrc/gk_icc.h): reads every file named on
// the command line as a profile and prints the parsed transform or the refusal, one line per file.
// Host code only; tests/test_icc.py builds it with -fsanitize=address,undefined and runs it over
// the accepted and the malformed profiles, so that a read outside a profile's bytes aborts it.
// The profile is copied into a heap block of exactly its size: the sanitizer sees the first byte
// past it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../grok_amd/csrc/gk_icc.h"

static const char* kind_name(const GkIccCurve& c) {
    return c.kind == GkIccCurve::IDENTITY ? "identity" : c.kind == GkIccCurve::PARA ? "para" : "table";
}

int main(int argc, char** argv) {
    int failed = 0;
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("%s: cannot open\n", argv[i]); failed = 1; continue; }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* buf = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);
        if (n > 0 && fread(buf, 1, (size_t)n, f) != (size_t)n) { printf("%s: cannot read\n", argv[i]); failed = 1; }
        fclose(f);
        GkIccTransform T;
        const std::string why = gk_icc_read(buf, (size_t)n, T);
        free(buf);
        if (!why.empty()) { printf("%s: refused: %s\n", argv[i], why.c_str()); continue; }
        printf("%s: ok: %s intent %u", argv[i], T.grey ? "grey" : "rgb", T.intent);
        for (int k = 0; k < (T.grey ? 1 : 3); ++k) {
            const GkIccCurve& c = T.curve[k];
            printf(" curve%d %s", k, kind_name(c));
            if (c.kind == GkIccCurve::PARA) printf("(g=%.6f a=%.6f b=%.6f c=%.6f d=%.6f e=%.6f f=%.6f)", c.g, c.a, c.b, c.c, c.d, c.e, c.f);
            if (c.kind == GkIccCurve::TABLE) printf("(%zu)", c.table.size());
            // every sample of an 8-bit and the ends and middle of a 16-bit image through the curve
            double s = 0;
            for (uint32_t v = 0; v < 256; ++v) s += c.eval(v, 255);
            s += c.eval(0, 65535) + c.eval(32768, 65535) + c.eval(65535, 65535);
            printf(" sum %.6f", s);
        }
        if (!T.grey)
            printf(" m [%.6f %.6f %.6f; %.6f %.6f %.6f; %.6f %.6f %.6f]", T.m[0][0], T.m[0][1], T.m[0][2], T.m[1][0], T.m[1][1],
                   T.m[1][2], T.m[2][0], T.m[2][1], T.m[2][2]);
        printf("\n");
    }
    return failed;
}
