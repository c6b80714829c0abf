// policy.h -- the A/B variables of DESIGN.md section 8 as one record (host only).
//
// A context runs under the environment it was created in: rau_create calls policy_from_env() once and keeps the
// record; every launch decision, every workspace size and every captured step of that context reads the record,
// never the environment.  policy_from_env() is the only function of the library that reads these variables.
// Kernel files know none of this: the context layer turns the record into the mode structs of kernels.h
// (conv_mode / att_mode / lin_mode below, with what the context adds: its dtype, its mode, its batch size).
#pragma once
#include <vector>

#include "kernels.h"

namespace rau {

// One field per variable.  An unset variable leaves its field at the initialiser: the constant default, or -1
// where the default is chosen by shape.  Presence-only variables count when set to any string.
struct Policy {
  // ---- 1x1 convolutions
  int conv_wide = 3;           // RAU_CONV_WIDE=mask: 1 i_embed forward, 2 ifeatproj forward
  int conv_wide_per_cu = 1;    // RAU_CONV_WIDE_PER_CU: anything but 2 means 1
  int conv_sample = 12;        // RAU_CONV_SAMPLE=mask (conv_sample_ok's `which`)
  int dgrad_dma = 3;           // RAU_DGRAD_DMA: 0 off, 2 ring of two stages, anything else three
  bool wgrad_dma_off = false;  // RAU_WGRAD_DMA_OFF
  bool wgrad16_off = false;    // RAU_WGRAD16_OFF
  int wgrad_groups = 0;        // RAU_WGRAD_GROUPS: 1 | 2, anything else 0 = by shape
  bool xd_f32 = false;         // RAU_XD_F32
  bool xgrad_fused = false;    // RAU_XGRAD_FUSED: non-zero
  // ---- attention
  bool att_split = false, att_fused = false;   // RAU_ATT_SPLIT, RAU_ATT_FUSED
  bool att_dma_off = false;    // RAU_ATT_DMA_OFF
  int att_chunks = 0;          // RAU_ATT_CHUNKS: 1..8, anything else 0 = by batch size
  int att_waves_fwd = 0, att_waves_bwd = 0;    // RAU_ATT_WAVES_FWD / _BWD: 8 | 16, anything else 0 = the caller's
  // ---- Linear GEMMs
  bool skinny_dma_off = false, skinny_ragged_off = false, skinny_align16 = false;   // RAU_SKINNY_*
  int skinny_deep = -1;        // RAU_SKINNY_DEEP: 0 | 1 (non-zero)
  // ---- schedule
  int seam = 3;                // RAU_SEAM=mask
  int wg_bulk = -1;            // RAU_WG_BULK=mask (negative: by shape)
  int side_split = -1;         // RAU_SIDE_SPLIT: 0 | 1 (non-zero)
  int enc_ws = -1;             // RAU_ENC_WS: 0 | 1 (non-zero)
  int enc_chunks = 0;          // RAU_ENC_CHUNKS: above 0, else the default count
  // RAU_HOP_GROUPS / RAU_BWD_GROUPS: the sizes as written; empty when unset or when an entry is below 1
  std::vector<int> hop_groups, bwd_groups;
};
Policy policy_from_env();
// `sizes` laid out over H hops, out[h] = n where hops [h, h + n) form a group and 0 elsewhere; empty (= ignored)
// unless the sizes sum to H
std::vector<int> hop_partition(const std::vector<int>& sizes, int H);

// The record as the launchers' modes.  bf16: the context's rau_dtype; light: conv_att_dgrad_dz's; eval: evaluate
// mode (16 forward waves: no conv tile is resident beside the hops); chain_bound: rau_ctx.h.
ConvMode conv_mode(const Policy& p, int bf16, bool light);
AttMode att_mode(const Policy& p, int bf16, bool eval);
LinMode lin_mode(const Policy& p, int bf16, bool chain_bound);

}  // namespace rau
