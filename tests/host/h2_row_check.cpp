// Prints what the host-compilable part of gif_amd/csrc/h2_row.h (the f16x2 row exponent, its guard statistics and the weight rows'
// exponent and flag) computes, one line per case; this program includes nothing else of the library.  Floats travel as their bit
// patterns.  Lines:
//   exp t=<target> m=<bits> -> e=<int>
//   lane <seq> <step> m=<bits> -> ex= dl= sc= lim= max= gmin= wide=     one lane of the wave-uniform form, as if some lane of the
//                                                                      wave always outgrew its exponent (the select decides per lane).
//                                                                      h2_observe itself (conv_common.h) is device code: its three
//                                                                      steps (h2_note, dl = 0, h2_grow) are REPEATED in sequence()
//                                                                      below, so a change of its body shows in the GPU bit tests only
//   priv <seq> <step> m0=<bits> m1=<bits> -> (the same fields) grew=   the private form: two groups under one decision
//   wide <name> g=<bits>,<bits>,... -> wide=                           a row's groups through the statistics alone
//   wrow rowmax=<bits> -> e=                                            weight row exponent
//   wnar rowmax=<bits> gm=<bits> -> narrow=                             weight row flag after one group
// tests/test_h2_row_cpu.py builds this with AddressSanitizer and UBSan (host code only), runs it and compares every line with
// tests/h2_row_ref.py.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define GIF_H2_FN inline
#include "h2_row.h"

namespace {

unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
float from_bits(unsigned u) { float v; memcpy(&v, &u, 4); return v; }

void print_state(const gif::H2Row& s) {
    printf("ex=%d dl=%d sc=%08x lim=%08x max=%08x gmin=%08x wide=%d", s.ex, s.dl, bits(s.sc), bits(s.lim), bits(s.max), s.gmin, (int)gif::h2_wide(s));
}

// every sequence through both forms; the private form sees each value once as the first and once as the second of its two groups,
// beside the previous value of the sequence halved (a second group that must not decide)
void sequence(const char* name, const std::vector<float>& ms) {
    gif::H2Row lane, priv;
    for (size_t k = 0; k < ms.size(); ++k) {
        const float m = ms[k];
        gif::h2_note(lane, m);
        lane.dl = 0;
        gif::h2_grow(lane, m);
        printf("lane %s %zu m=%08x -> ", name, k, bits(m));
        print_state(lane);
        printf("\n");
        const float other = k ? 0.5f * ms[k - 1] : 0.f;
        const float m0 = k % 2 ? other : m, m1 = k % 2 ? m : other;
        const bool grew = gif::h2_observe_private(priv, m0, m1);
        printf("priv %s %zu m0=%08x m1=%08x -> ", name, k, bits(m0), bits(m1));
        print_state(priv);
        printf(" grew=%d\n", (int)grew);
    }
}

void wide_row(const char* name, const std::vector<float>& groups) {
    gif::H2Row s;
    printf("wide %s g=", name);
    for (size_t k = 0; k < groups.size(); ++k) {
        gif::h2_note(s, groups[k]);
        printf("%s%08x", k ? "," : "", bits(groups[k]));
    }
    printf(" -> wide=%d\n", (int)gif::h2_wide(s));
}

}  // namespace

int main() {
    // ---- h2_exp_for: both targets, every exponent field, smallest / next / largest mantissa
    const unsigned mant[3] = {0u, 1u, 0x7fffffu};
    for (int t : {gif::kH2Target, gif::kH2TargetW})
        for (unsigned f = 0; f < 256; ++f)
            for (unsigned mt : mant) printf("exp t=%d m=%08x -> e=%d\n", t, (f << 23) | mt, gif::h2_exp_for((f << 23) | mt, t));

    // ---- tracker sequences (all from the initial state, ex = 126)
    sequence("first", {1.f});
    sequence("headroom_in", {1.f, 3.f, 7.99f, 1.5f});          // growth by less than the 4x headroom: no new exponent
    sequence("headroom_out", {1.f, 9.f, 100.f, 1.0e6f});       // growth beyond it
    {
        gif::H2Row s;
        gif::h2_grow(s, 1.f);  // lim of the exponent chosen for 1.0
        sequence("at_lim", {1.f, s.lim, nextafterf(s.lim, INFINITY), s.lim});  // m == lim keeps the exponent, the next float does not
    }
    sequence("ties", {2.f, 2.f, 2.f, 16.f, 16.f});
    sequence("zeros_between", {0.f, 0.f, 1.f, 0.f, 0.f, 0.5f, 0.f, 40.f, 0.f});
    sequence("tiny", {1.0e-38f, 3.0e-38f, 1.0e-40f, from_bits(1u), 1.0e-38f, 1.17549435e-38f});  // around the smallest normal float
    sequence("huge", {1.0e30f, 3.0e30f, 1.0e38f, 3.0e38f});
    sequence("tiny_then_huge", {1.0e-38f, 1.0e30f});
    sequence("shrinking", {1000.f, 10.f, 0.1f, 1.0e-5f, 1.0e-20f, 0.f, 999.f});  // the exponent never goes back
    sequence("all_zero", {0.f, 0.f, 0.f});

    // ---- window test: smallest non-zero group 13, 14, 15 exponent steps below the row maximum
    for (int d : {13, 14, 15}) {
        char name[32];
        snprintf(name, sizeof name, "below_%d", d);
        wide_row(name, {1.f, ldexpf(1.f, -d), 0.25f});
        snprintf(name, sizeof name, "below_%d_mant", d);  // the distance is one of exponent fields: mantissas do not matter
        wide_row(name, {1.9999999f, ldexpf(1.f, -d), 0.f, ldexpf(1.9999999f, -d)});
        snprintf(name, sizeof name, "below_%d_first", d);  // the small group comes first
        wide_row(name, {ldexpf(3.f, 20 - d), 0.f, ldexpf(3.f, 20)});
    }
    wide_row("only_zero", {0.f, 0.f, 0.f, 0.f});
    wide_row("zeros_one_value", {0.f, 0.f, 5.f, 0.f});
    wide_row("zeros_one_tiny", {0.f, 1.0e-30f, 0.f});
    wide_row("denormal_group", {1.f, 1.0e-40f});

    // ---- weight side
    for (float rm : {0.f, 1.0e-40f, 1.0e-38f, 0.003f, 1.f, 1.9999999f, 2.f, 700.f, 1.0e30f, 3.0e38f}) printf("wrow rowmax=%08x -> e=%d\n", bits(rm), gif::h2_weight_exp(rm));
    for (float rm : {1.f, 1.9999999f, 0.003f})
        for (int d : {0, 15, 16, 17, 40}) {
            for (float gm : {ldexpf(rm, -d), ldexpf(1.f, -d) * 1.5f, 0.f}) {
                bool narrow = false;
                gif::h2_weight_note(rm, gm, narrow);
                printf("wnar rowmax=%08x gm=%08x -> narrow=%d\n", bits(rm), bits(gm), (int)narrow);
            }
        }
    bool kept = true;  // a raised flag stays raised
    gif::h2_weight_note(1.f, 1.f, kept);
    printf("wnar_kept -> narrow=%d\n", (int)kept);
    return 0;
}
