// Stand-alone host program over gif_amd/csrc/flame_chain.h alone (tests/test_flame_chain_cpu.py builds and runs it): for a list of
// chains and poses it prints the inputs and what the header's functions return, every float as its 8 hex digits, one case per block:
//   case <name> J=<J> parents=<p0,..>
//   jt / r / gA / gF <floats>          the inputs: joints [J][3], axis-angles [J][3], g_A [J][12], g_F [J-1][9]
//   gjt / gr <floats>                  the outputs: dL/d joints, dL/d axis-angles
// The test recomputes gjt and gr from the inputs with float64 autograd.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define GIF_CHAIN_FN inline
#include "flame_chain.h"

namespace {

constexpr int kJ = 8;
uint32_t state = 12345u;

float uniform() {  // in (-1, 1), a 24-bit LCG draw
    state = state * 1664525u + 1013904223u;
    return (float)((state >> 8) & 0xffffffu) / 8388608.f - 1.f;
}

void put(const char* name, const float* v, int n) {
    printf("%s", name);
    for (int i = 0; i < n; ++i) {
        uint32_t bits;
        memcpy(&bits, &v[i], 4);
        printf(" %08x", bits);
    }
    printf("\n");
}

// pose: 0 random rotations of up to ~0.6 rad, 1 exact zeros, 2 an angle within 1e-3 of pi, 3 an angle of 1e-6,
//       4 one of each: joint 0 zeros, joint 1 near pi, joint 2 tiny, random beyond
void run(const char* name, int J, const int* parents, int pose) {
    float jt[3 * kJ], r[3 * kJ], gA[12 * kJ], gF[9 * kJ], R[9 * kJ], GR[9 * kJ], gR[9 * kJ], gGt[3 * kJ], gjt[3 * kJ], gr[3 * kJ];
    for (int i = 0; i < 3 * J; ++i) jt[i] = 0.3f * uniform();
    for (int j = 0; j < J; ++j) {
        float d[3] = {uniform(), uniform(), uniform()};
        float n = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (n < 1e-3f) { d[0] = 1.f; n = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); }
        const int kind = pose == 4 ? (j < 3 ? 1 + j : 0) : pose;
        const float angle = kind == 0 ? 0.6f * (0.5f + 0.5f * uniform()) + 0.05f : kind == 2 ? 3.14159265f - 5e-4f : kind == 3 ? 1e-6f : 0.f;
        for (int i = 0; i < 3; ++i) r[3 * j + i] = kind == 1 ? 0.f : d[i] / n * angle;
    }
    for (int i = 0; i < 12 * J; ++i) gA[i] = uniform();
    for (int i = 0; i < 9 * (J - 1); ++i) gF[i] = uniform();
    for (int j = 0; j < J; ++j) gif::chain_rodrigues(r + 3 * j, R + 9 * j);
    gif::chain_world_rotations(J, parents, R, GR);
    gif::chain_reverse(J, parents, jt, R, GR, gA, J > 1 ? gF : nullptr, gR, gGt, gjt);
    for (int j = 0; j < J; ++j) gif::chain_rodrigues_bwd(r + 3 * j, gR + 9 * j, gr + 3 * j);
    printf("case %s J=%d parents=", name, J);
    for (int j = 0; j < J; ++j) printf("%s%d", j ? "," : "", parents[j]);
    printf("\n");
    put("jt", jt, 3 * J);
    put("r", r, 3 * J);
    put("gA", gA, 12 * J);
    put("gF", gF, 9 * (J - 1));
    put("gjt", gjt, 3 * J);
    put("gr", gr, 3 * J);
}

}  // namespace

int main() {
    const int root[1] = {-1}, chain[3] = {-1, 0, 1}, flame[5] = {-1, 0, 1, 1, 1}, eight[8] = {-1, 0, 1, 1, 1, 0, 5, 2};
    const int forest[5] = {-1, 0, -1, 2, 2};  // two roots
    run("j1", 1, root, 0);
    run("j3_chain", 3, chain, 0);
    run("j5_flame", 5, flame, 0);
    run("j8", 8, eight, 0);
    run("j5_forest", 5, forest, 0);
    run("j1_zero", 1, root, 1);
    run("j3_zero", 3, chain, 1);
    run("j5_zero", 5, flame, 1);
    run("j3_near_pi", 3, chain, 2);
    run("j5_near_pi", 5, flame, 2);
    run("j3_tiny", 3, chain, 3);
    run("j5_tiny", 5, flame, 3);
    run("j5_mixed", 5, flame, 4);
    run("j8_mixed", 8, eight, 4);
    return 0;
}
