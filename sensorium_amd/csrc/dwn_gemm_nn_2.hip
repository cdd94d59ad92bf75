// gemm_nn_kernel instantiations, part 2 of 6: the launch_nn_t combinations below and every kernel they launch are compiled
// here and nowhere else (dwn_gemm_nn.h: NN_COMBOS).  The parts are balanced by measured compile time
// (profiles/gemm_split_build.txt), not by theme.
#include "dwn_gemm_nn.h"

NN_INSTANTIATE(float, LD_PLAIN, EPI_DH3)
NN_INSTANTIATE(bf16_t, LD_BNACT, EPI_READOUT)
NN_INSTANTIATE(bf16_t, LD_GATE, EPI_STORE)
