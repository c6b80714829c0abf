// policy.hip -- policy_from_env(): the one reader of the A/B variables (policy.h).
#include "policy.h"

#include <cstdlib>

namespace rau {

namespace {
bool is_set(const char* name) { return std::getenv(name) != nullptr; }
int int_or(const char* name, int unset) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : unset;
}
int flag_or(const char* name, int unset) {   // 0 | 1 (non-zero)
  const char* e = std::getenv(name);
  return e ? (std::atoi(e) != 0 ? 1 : 0) : unset;
}
int one_of(const char* name, int a, int b) {   // a | b, anything else 0
  const int v = int_or(name, 0);
  return (v == a || v == b) ? v : 0;
}
std::vector<int> size_list(const char* name) {
  std::vector<int> sizes;
  const char* e = std::getenv(name);
  for (const char* q = e ? e : ""; *q;) {
    const int v = std::atoi(q);
    if (v < 1) return {};
    sizes.push_back(v);
    while (*q && *q != ',') ++q;
    if (*q == ',') ++q;
  }
  return sizes;
}
}  // namespace

Policy policy_from_env() {
  Policy p;
  p.conv_wide = int_or("RAU_CONV_WIDE", p.conv_wide);
  p.conv_wide_per_cu = int_or("RAU_CONV_WIDE_PER_CU", 1) == 2 ? 2 : 1;
  p.conv_sample = int_or("RAU_CONV_SAMPLE", p.conv_sample);
  p.dgrad_dma = int_or("RAU_DGRAD_DMA", p.dgrad_dma);
  p.wgrad_dma_off = is_set("RAU_WGRAD_DMA_OFF");
  p.wgrad16_off = is_set("RAU_WGRAD16_OFF");
  p.wgrad_groups = one_of("RAU_WGRAD_GROUPS", 1, 2);
  p.xd_f32 = is_set("RAU_XD_F32");
  p.xgrad_fused = int_or("RAU_XGRAD_FUSED", 0) != 0;
  p.att_split = is_set("RAU_ATT_SPLIT");
  p.att_fused = is_set("RAU_ATT_FUSED");
  p.att_dma_off = is_set("RAU_ATT_DMA_OFF");
  const int nc = int_or("RAU_ATT_CHUNKS", 0);
  p.att_chunks = (nc >= 1 && nc <= 8) ? nc : 0;
  p.att_waves_fwd = one_of("RAU_ATT_WAVES_FWD", 8, 16);
  p.att_waves_bwd = one_of("RAU_ATT_WAVES_BWD", 8, 16);
  p.skinny_dma_off = is_set("RAU_SKINNY_DMA_OFF");
  p.skinny_ragged_off = is_set("RAU_SKINNY_RAGGED_OFF");
  p.skinny_align16 = is_set("RAU_SKINNY_ALIGN16");
  p.skinny_deep = flag_or("RAU_SKINNY_DEEP", -1);
  p.seam = int_or("RAU_SEAM", p.seam);
  p.wg_bulk = int_or("RAU_WG_BULK", -1);
  p.side_split = flag_or("RAU_SIDE_SPLIT", -1);
  p.enc_ws = flag_or("RAU_ENC_WS", -1);
  p.enc_chunks = int_or("RAU_ENC_CHUNKS", 0);
  p.hop_groups = size_list("RAU_HOP_GROUPS");
  p.bwd_groups = size_list("RAU_BWD_GROUPS");
  return p;
}

std::vector<int> hop_partition(const std::vector<int>& sizes, int H) {
  int sum = 0;
  for (int n : sizes) sum += n;
  if (sizes.empty() || sum != H) return {};
  std::vector<int> out(H, 0);
  int h0 = 0;
  for (int n : sizes) { out[h0] = n; h0 += n; }
  return out;
}

ConvMode conv_mode(const Policy& p, int bf16, bool light) {
  ConvMode m;
  m.bf16 = bf16;
  m.light = light ? 1 : 0;
  m.wide = p.conv_wide;
  m.wide_per_cu = p.conv_wide_per_cu;
  m.sample = p.conv_sample;
  m.dgrad_ring = p.dgrad_dma == 0 ? 0 : p.dgrad_dma == 2 ? 2 : 3;
  m.wgrad_dma = !p.wgrad_dma_off;
  m.wgrad16 = !p.wgrad16_off;
  m.wgrad_groups = p.wgrad_groups;
  return m;
}

AttMode att_mode(const Policy& p, int bf16, bool eval) {
  AttMode m;
  m.dma = !p.att_dma_off;
  m.waves_fwd = p.att_waves_fwd ? p.att_waves_fwd : eval ? 16 : 8;
  m.waves_bwd = p.att_waves_bwd ? p.att_waves_bwd : bf16 ? 8 : 16;
  m.chunks = p.att_chunks;
  return m;
}

LinMode lin_mode(const Policy& p, int bf16, bool chain_bound) {
  LinMode m;
  m.bf16 = bf16 == 1;
  m.deep = p.skinny_deep >= 0 ? p.skinny_deep : (chain_bound ? 1 : 0);
  m.dma = !p.skinny_dma_off;
  m.ragged = !p.skinny_ragged_off;
  m.align16 = p.skinny_align16;
  return m;
}

}  // namespace rau
