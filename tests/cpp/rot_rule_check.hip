// rot_rule_check.hip -- the host instantiation of orbm::three_maxima (orbslamm_amd/csrc/orbm_kernels.hip), the one statement of
// ComputeThreeMaxima that every pruning kernel calls through its wave form; no device, no HIP runtime call.  Reads histograms of
// thirty counts from standard input (thirty integers each, any white space between them) and prints the three indices of each on
// a line; tests/test_rot_rule_cpu.py holds them to the oracle's orc_three_maxima.
//   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -o rot_rule_check tests/cpp/rot_rule_check.hip && ./rot_rule_check < histograms
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../orbslamm_amd/csrc/orbm_kernels.hip"

int main()
{
    int h[orbm::kHistoLength];
    for (;;) {
        for (int i = 0; i < orbm::kHistoLength; i++)
            if (std::scanf("%d", &h[i]) != 1) return i == 0 ? 0 : 1;   // (a partial histogram is an error)
        int ind1, ind2, ind3;
        orbm::three_maxima([&h](int i) { return h[i]; }, ind1, ind2, ind3);
        std::printf("%d %d %d\n", ind1, ind2, ind3);
    }
}
