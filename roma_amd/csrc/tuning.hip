// The switch table (tuning.h).  Host code only.  Adding a switch: one enumerator in tuning.h, one row here, and
// tuning(SW_...) at the site that uses it; roma_tuning, roma_tuning_describe and the documents' table follow from the row.
#include "tuning.h"

#include <stdlib.h>
#include <string.h>

#include "../../include/roma_hip.h"

namespace roma {
void set_error(const std::string& msg);  // api.hip; declared here, not through common.h: this file needs no HIP header
namespace {

struct Row {
  Switch id;
  const char* key;  // roma_tuning key, or nullptr
  const char* env;  // environment variable, or nullptr
  long def;
  int floor;        // lowest value that counts as an override (anything below clears it)
  const char* doc;
};

constexpr Row ROWS[] = {
    {SW_GEMM8P, "gemm8p", "ROMA_GEMM8P", 1, 0, "large bf16 GEMMs on the 8-phase 256 x 256 kernel (1) or on the one-barrier-per-slab kernel (0)"},
    {SW_GEMM_DBG, "gemm_dbg", "ROMA_GEMM_DBG", 0, 0, "experiment bits of the GEMM kernels (1 skip output stores, 2 skip the K loop, 2048 no streaming stores, ...)"},
    {SW_GEMM8P_WALK, "gemm8p_walk", nullptr, -1, 1, "gemm8p: tile rows per group of the persistent walk (1 = row major); unset = 8 from 24 tile columns on, else 1"},
    {SW_GEMM8P_SCHED, "gemm8p_sched", "ROMA_GEMM8P_SCHED", 1, 0, "gemm8p K-loop schedule: 1 k-half phases, 0 quadrant phases (tools builds only)"},
    {SW_GEMM8P_MAXWG, "gemm8p_maxwg", nullptr, -1, 8, "gemm8p, measurement only: cap the persistent grid at n workgroups (a multiple of 8); unset = one per CU"},
    {SW_WS1X1, "ws1x1", "ROMA_WS1X1", 1, 0, "N = K = 576 refiner 1x1 on the weight-stationary kernel (1) or on the 256 x 192 tile kernel (0)"},
    {SW_LC_MODE, "lc_mode", "ROMA_LC_MODE", 0, 0, "local correlation: 0 tiled form + gather work list, 1 every tile on the gather list (key only), 2 per-pixel kernel"},
    {SW_LC_BIN, "lc_bin", "ROMA_LC_BIN", 1, 0, "local correlation: queries of incoherent tiles sorted by target bin, counters in LDS (1) or device atomics (2), or gathered per query (0)"},
    {SW_CONV64, "conv64", "ROMA_CONV64", 7, 0, "weight-stationary VGG front end, bit mask: 1 the Cin = 64 kernels, 2 the Cin = 128 kernel, 4 the fused first layer"},
    {SW_CONV_PATCH, "conv_patch", "ROMA_CONV_PATCH", 1, 0, "patch-resident 3x3 kernel for slab-major VGG layers (1) or gemm8p (0); environment 0 also packs tap-major weights"},
    {SW_ATTN_XCD, "attn_xcd", "ROMA_ATTN_XCD", 1, 0, "attention work items in per-XCD bands of (batch, head) (1) or in plain order (0)"},
    {SW_ATTN_EXP2, "attn_exp2", nullptr, -1, 0, "tools only: force the 2^x softmax of the 16-bit attention kernel on / off; unset = as the caller says"},
    {SW_DW_RING, "dw_ring", "ROMA_DW_RING", 1, 0, "depthwise 5x5: 0 register-prefetch kernel, 1 ring kernel for the large launches, 2 ring kernel for every shape it takes"},
    {SW_GP_COL, "gp_col", "ROMA_GP_COL", 1, 0, "GP Cholesky left-looking, one launch per block column (1) or the right-looking launch chain (0)"},
    {SW_POOL_PROJ, "pool_proj", "ROMA_POOL_PROJ", 1, 0, "max-pool + proj head of strides 1 / 2 in one pass (1) or as separate kernels (0)"},
    {SW_GP_COL_LEADER, "gp_col_leader", "ROMA_GP_COL_LEADER", 1, 0, "block-column Cholesky: a leader workgroup factorises the diagonal block, its product formed one launch ahead (1) or in its own launch (2), or every workgroup its own copy (0)"},
    {SW_GEMM8P_MINM, nullptr, "ROMA_GEMM8P_MINM", 2048, 0, "gemm8p: smallest M it takes for the wide (N >= 2048) dense launches"},
    {SW_GEMM_NT, nullptr, "ROMA_GEMM_NT", 1, 0, "non-temporal output stores in the 16-bit GEMM row writer"},
    {SW_GEMM_F32_FILL, nullptr, "ROMA_GEMM_F32_FILL", 1, 0, "exact-f32 GEMMs below 192 tiles of 256 x 256 run on 128 x 128 tiles"},
    {SW_GEMM_SMALLM, nullptr, "ROMA_GEMM_SMALLM", 1, 0, "GEMMs below 320 tiles of 128 x 128 run on 128 x 64 tiles"},
    {SW_CONV64_SY, nullptr, "ROMA_CONV64_SY", 0, 0, "conv64 strip height in rows; 0 = the split of H with the fewest rounds"},
    {SW_CONV_KORDER, nullptr, "ROMA_CONV_KORDER", 1, 0, "VGG layers with Cout >= 256 pack slab-major weight rows (read when a handle is created)"},
    {SW_RB_SY, nullptr, "ROMA_RB_SY", 0, 0, "fused refiner block strip height in rows; 0 = the split of H with the fewest rounds"},
    {SW_DWR_MAXSY, nullptr, "ROMA_DWR_MAXSY", 1 << 20, 0, "depthwise ring kernel: cap of the strip height in rows (at least 6)"},
    {SW_DW_RING_MINELEMS, nullptr, "ROMA_DW_RING_MINELEMS", 64l << 20, 0, "dw_ring = 1: smallest launch, in elements, that goes to the ring kernel"},
    {SW_RI_VEC, nullptr, "ROMA_RI_VEC", 1, 0, "refiner_input on the 16-byte vector kernel where alignment allows"},
    {SW_OUT_ROW, nullptr, "ROMA_OUT_ROW", 1, 0, "refiner_out: row kernel for C = 24 in 16-bit storage"},
    {SW_OUT_LPR, nullptr, "ROMA_OUT_LPR", 1, 0, "refiner_out, 16-bit: lanes per row chosen to fill the 16-byte pieces best"},
    {SW_OUT_ROWS_IT, nullptr, "ROMA_OUT_ROWS_IT", 0, 0, "refiner_out: row groups per wave (even, >= 2); otherwise 8"},
    {SW_GP_AUG, nullptr, "ROMA_GP_AUG", 1, 0, "GP Cholesky: right-hand sides stored behind A ride along the factorisation (0 = separate forward loop)"},
    {SW_GP_BWD2, nullptr, "ROMA_GP_BWD2", 1, 0, "GP Cholesky: backward substitution with one launch per step (0 = two)"},
    {SW_COMPOSE_OUT, nullptr, "ROMA_COMPOSE_OUT", 1, 0, "initial value of the handle option compose_out_conv (read when a handle is created)"},
    {SW_VIT_RES_F32, nullptr, "ROMA_VIT_RES_F32", 0, 0, "force DINOv2's f32 residual stream in the 16-bit modes"},
    {SW_STREAMS, nullptr, "ROMA_STREAMS", 0, 0, "number of sub-batch streams of match(); 0 = the handle's option"},
    {SW_STREAMS_SERIAL, nullptr, "ROMA_STREAMS_SERIAL", 0, 0, "diagnostic: sub-batch streams run one after the other"},
    {SW_DEBUG_DUAL_SLOT, nullptr, "ROMA_DEBUG_DUAL_SLOT", -1, 0, "diagnostic: keep the stream split in debug mode, sub-batch k captures the stages of ROMA_DEBUG_ONLY"},
};
constexpr int NROWS = sizeof(ROWS) / sizeof(ROWS[0]);
constexpr bool rows_in_enum_order() {
  for (int i = 0; i < NROWS; ++i)
    if (ROWS[i].id != i) return false;
  return true;
}
static_assert(NROWS == SW_COUNT && rows_in_enum_order(), "one row per Switch, in enum order");
constexpr bool json_plain(const char* s) {  // tuning_describe writes the strings unescaped
  for (; s && *s; ++s)
    if (*s == '"' || *s == '\\' || *s < ' ') return false;
  return true;
}
constexpr bool rows_json_plain() {
  for (const Row& r : ROWS)
    if (!json_plain(r.key) || !json_plain(r.env) || !json_plain(r.doc)) return false;
  return true;
}
static_assert(rows_json_plain(), "keys, environment names and docs: plain ASCII without quote, backslash or control character");

struct Overrides {
  long v[SW_COUNT];
  constexpr Overrides() : v{} {
    for (long& x : v) x = -1;
  }
};
[[clang::require_constant_initialization]] Overrides g_override;

struct Env {
  long v[SW_COUNT];
  Env() {
    for (int i = 0; i < NROWS; ++i) {
      const char* s = ROWS[i].env ? getenv(ROWS[i].env) : nullptr;
      // atol for every row: most sites used atoi before the table, which is (int)strtol - the site's narrowing gives the same int
      v[i] = s ? atol(s) : ROWS[i].def;
    }
  }
};
const Env& env() {
  static const Env e;  // parsed at the first use of the table, thread-safe; later calls pay the guard's flag load
  return e;
}

}  // namespace

long tuning_env(Switch id) { return env().v[id]; }
long tuning_override(Switch id) { return g_override.v[id] >= ROWS[id].floor ? g_override.v[id] : -1; }
long tuning(Switch id) { return g_override.v[id] >= ROWS[id].floor ? g_override.v[id] : tuning_env(id); }

int tuning_set(const char* key, long value) {
  for (const Row& r : ROWS)
    if (r.key && !strcmp(r.key, key)) {
      g_override.v[r.id] = value >= r.floor ? value : -1;
      return 0;
    }
  set_error(std::string("roma_tuning: unknown key ") + key);
  return ROMA_ERR_ARG;
}

std::string tuning_describe() {
  std::string js = "[";
  for (const Row& r : ROWS) {
    const auto quoted = [](const char* s) { return s ? "\"" + std::string(s) + "\"" : std::string("null"); };
    const long ov = tuning_override(r.id);
    js += std::string(r.id ? ", " : "") + "{\"key\": " + quoted(r.key) + ", \"env\": " + quoted(r.env) +
          ", \"default\": " + std::to_string(r.def) + ", \"override\": " + (ov >= 0 ? std::to_string(ov) : "null") +
          ", \"value\": " + std::to_string(tuning(r.id)) + ", \"doc\": " + quoted(r.doc) + "}";
  }
  return js + "]";
}

}  // namespace roma
