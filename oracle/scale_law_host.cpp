// Stand-alone host program over csrc/scale_law.hpp: the functions the device kernels call, compiled for the CPU, so that the
// C++ statement of the slot law can be pinned against oracle/scale_ref.py without a GPU (tests/test_f16_scale_law_host.py) and
// run under the host sanitizers (make -C oracle scale_law_asan).
//
// stdin, one request per line, every float as the 8 hex digits of its bits:
//     F <|max|> <scale> <floor>      -> "<scale'> <floor'> <flag>"      (finish_slot)
//     R <m> <|max| now> <floor>      -> "<0 or 1>"                      (should_report)
// stdout: one answer line per request.  Exit status 2 on a line it cannot read.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "scale_law.hpp"

static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static uint32_t to_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    char line[128];
    while (std::fgets(line, sizeof line, stdin)) {
        char op;
        unsigned a, b, c;
        if (std::sscanf(line, " %c %x %x %x", &op, &a, &b, &c) != 4 || (op != 'F' && op != 'R')) {
            std::fprintf(stderr, "scale_law_host: bad line: %s", line);
            return 2;
        }
        if (op == 'F') {
            const ebfi::SlotUpdate u = ebfi::finish_slot(from_bits(a), from_bits(b), from_bits(c));
            std::printf("%08x %08x %d\n", to_bits(u.scale), to_bits(u.floor), u.flag);
        } else {
            std::printf("%d\n", ebfi::should_report(from_bits(a), from_bits(b), from_bits(c)) ? 1 : 0);
        }
    }
    return 0;
}
