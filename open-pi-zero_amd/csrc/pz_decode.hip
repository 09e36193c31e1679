// Decode-shaped joint attention for the denoise steps (pizero.py:461-481 with joint_model.py:130-304): the entry
// points of the kernels in pz_decode_kernels.h, instantiated without the log-sum-exp export (pz_expert_attn.hip
// holds the instantiation with it, for training).
#include "pz_decode_kernels.h"

extern "C" int64_t pz_decode_attn_ws_bytes(int64_t B, int64_t rows, int64_t nk) {
  const int64_t rpad = (rows + DA_R - 1) / DA_R * DA_R;
  return B * ((nk + DA_KC - 1) / DA_KC) * rpad * DA_RS * (int64_t)sizeof(float);
}

extern "C" int pz_decode_attn(const pz_decode_attn_args* a, void* stream) { return da_launch<false>(a, nullptr, stream); }
