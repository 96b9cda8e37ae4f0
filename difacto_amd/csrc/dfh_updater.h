// dfh_updater.h — SGDUpdater::Update for one key, in registers (src/sgd/sgd_updater.cc): FTRL on w, AdaGrad on a V
// coordinate, and the values InitV writes — the hash of (key, coordinate) by default, the reference's rand_r chain in
// parity mode (REFRAND).  Device functions only; the backward roles (dfh_backward.hip), k_update_fused (dfh_update.hip),
// the owner side of the store (dfh_owner.hip), the lookup passes (dfh_lookup.hip) and the warm start (dfh_index.hip) apply
// them.  hash_init_value stands here, not with the key index, because the row initialisers below need it.
#ifndef DFH_UPDATER_H_
#define DFH_UPDATER_H_
#include "dfh_device.h"

namespace dfh {

// The sharding-independent V init: must match oracle/difacto_oracle.c:orc_hash_init_value
__device__ __forceinline__ float hash_init_value(uint64_t key, int j, unsigned seed, float scale) {
  uint64_t a = splitmix64(key ^ (0xD1B54A32D192ED03ULL * ((uint64_t)seed + 1ULL)));
  uint64_t h = splitmix64(a + (uint64_t)j);
  uint32_t r = (uint32_t)(h >> 40);
  float u = (float)r * (1.0f / 16777216.0f);
  return (u - 0.5f) * scale;
}

// ---------------------------------------------------------------------------
// The per-key update arithmetic, kept operation-for-operation with
// src/sgd/sgd_updater.cc (no FMA contraction: the reference is built for
// generic x86-64 where a*b+c rounds twice).
// ---------------------------------------------------------------------------
#pragma clang fp contract(off)

// SGDUpdater::UpdateW — FTRL-proximal, src/sgd/sgd_updater.cc:104-120.
// returns the new w; hdr fields are updated in registers by the caller.
__device__ __forceinline__ float ftrl_update_w(float gw, float w, float& sqrt_g, float& z,
                                               const dfh_updater_param& P) {
  float sg = sqrt_g;
  gw += w * P.l2;                       // :108
  float nsg = sqrtf(sg * sg + gw * gw); // :109
  sqrt_g = nsg;
  z -= gw - (nsg - sg) / P.lr * w;      // :111
  float l1 = P.l1;
  if (z <= l1 && z >= -l1) return 0.0f; // :115-116
  float eta = (P.lr_beta + nsg) / P.lr; // :118
  return (z > 0 ? z - l1 : z + l1) / eta; // :119
}

// SGDUpdater::UpdateV — AdaGrad, one coordinate, src/sgd/sgd_updater.cc:129-138, operation for
// operation (IEEE-rounded square root and division, no contraction): given the same gradient the
// new V and accumulator are the reference's, bit for bit.  -DDFH_FAST_ADAGRAD swaps in the hardware
// v_sqrt_f32 / v_rcp_f32 approximations (1 ulp each) for A/B timing of the update kernel only.
__device__ __forceinline__ void adagrad_update_v(float gv, float& v, float& acc, const dfh_updater_param& P) {
  float g = gv + P.V_l2 * v;           // :132
  float cg = acc;                      // :133
#ifdef DFH_FAST_ADAGRAD
  float ncg = __builtin_amdgcn_sqrtf(cg * cg + g * g);
  float eta = P.V_lr * __builtin_amdgcn_rcpf(ncg + P.V_lr_beta);
#else
  float ncg = sqrtf(cg * cg + g * g);  // :134
  float eta = P.V_lr / (ncg + P.V_lr_beta);  // :135
#endif
  acc = ncg;
  v -= eta * g;                        // :136
}

// the reference's REFRAND value: (rand_r(&seed) / (real_t)RAND_MAX - 0.5) * scale  (:144)
__device__ __forceinline__ uint32_t lcg_step(uint32_t x) { return x * 1103515245u + 12345u; }
__device__ __forceinline__ float refrand_value(uint32_t& state, float scale) {
  // glibc rand_r: 3 LCG steps, 11+10+10 bits
  uint32_t next = lcg_step(state);
  int result = (int)((next / 65536u) % 2048u);
  next = lcg_step(next);
  result = (result << 10) ^ (int)((next / 65536u) % 1024u);
  next = lcg_step(next);
  result = (result << 10) ^ (int)((next / 65536u) % 1024u);
  state = next;
  float q = (float)result / 2147483648.0f;  // (real_t)RAND_MAX == 2^31 in float
  return (float)(((double)q - 0.5) * (double)scale);
}

#pragma clang fp contract(fast)

// LCG jump-ahead: state after n steps, by squaring the affine map x -> a x + c
__device__ __forceinline__ uint32_t lcg_jump(uint32_t x, uint64_t n) {
  uint32_t a = 1103515245u, c = 12345u;  // current power of the map
  uint32_t ra = 1u, rc = 0u;             // accumulated map (identity)
  while (n) {
    if (n & 1) {
      ra = ra * a;
      rc = rc * a + c;
    }
    c = c * a + c;
    a = a * a;
    n >>= 1;
  }
  return ra * x + rc;
}

// write V (hash init) + zero accumulators for row r; one thread does the row.  Rare (once per key).
__device__ __forceinline__ void init_v_hash_row(const TableView& t, uint32_t r, uint64_t key) {
  float* va = t.va + (size_t)r * (2 * t.kp);
  for (int j = 0; j < t.kp; ++j) {
    va[j] = j < t.k ? hash_init_value(key, j, t.p.seed, t.p.V_init_scale) : 0.0f;
    va[t.kp + j] = 0.0f;
  }
}

// the same for one lane's 16 B slice (coordinates d .. d + 3, d < kp) of a row that a whole lane group initialises
__device__ __forceinline__ void init_v_hash_slice(const TableView& t, uint32_t r, uint64_t key, int d) {
  float* va = t.va + (size_t)r * (2 * t.kp);
  float4 nv;
  nv.x = d + 0 < t.k ? hash_init_value(key, d + 0, t.p.seed, t.p.V_init_scale) : 0.0f;
  nv.y = d + 1 < t.k ? hash_init_value(key, d + 1, t.p.seed, t.p.V_init_scale) : 0.0f;
  nv.z = d + 2 < t.k ? hash_init_value(key, d + 2, t.p.seed, t.p.V_init_scale) : 0.0f;
  nv.w = d + 3 < t.k ? hash_init_value(key, d + 3, t.p.seed, t.p.V_init_scale) : 0.0f;
  st4(va + d, nv);
  st4(va + t.kp + d, make_float4(0.f, 0.f, 0.f, 0.f));
}

}  // namespace dfh
#endif  // DFH_UPDATER_H_
