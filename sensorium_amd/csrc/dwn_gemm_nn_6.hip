// gemm_nn_kernel instantiations, part 6 of 6: the launch_nn_t combinations below and every kernel they launch are compiled
// here and nowhere else (dwn_gemm_nn.h: NN_COMBOS).  The parts are balanced by measured compile time
// (profiles/gemm_split_build.txt), not by theme.
#include "dwn_gemm_nn.h"

NN_INSTANTIATE(float, LD_BNACT, EPI_STORE)
NN_INSTANTIATE(float, LD_AFFINE2, EPI_STORE)
NN_INSTANTIATE(float, LD_GATE, EPI_STORE)
NN_INSTANTIATE(bf16_t, LD_PLAIN, EPI_READOUT)
NN_INSTANTIATE(bf16_t, LD_PLAIN, EPI_READOUT_LB)
NN_INSTANTIATE(bf16_t, LD_PE, EPI_STORE)
