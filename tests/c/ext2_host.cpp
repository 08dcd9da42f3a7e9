// The host side of csrc/ext2.hpp, built with the host compiler alone (tests/test_ext2_host.py):
// reads lines "a0 a1 b0 b1" of u64 words, which need not be canonical, and prints
// "mul(a, b).c0 mul(a, b).c1 norm(a) times7(a0)", canonical, for each.
#include <inttypes.h>
#include <stdio.h>

#include "../../era-boojum_amd/csrc/ext2.hpp"

int main() {
    uint64_t a0, a1, b0, b1;
    while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a0, &a1, &b0, &b1) == 4) {
        const bj::ext2::E2 a = {a0, a1}, b = {b0, b1};
        const bj::ext2::E2 m = bj::ext2::mul(a, b);
        printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", gl::canon(m.c0), gl::canon(m.c1),
               gl::canon(bj::ext2::norm(a)), gl::canon(bj::ext2::times7(a0)));
    }
    return 0;
}
