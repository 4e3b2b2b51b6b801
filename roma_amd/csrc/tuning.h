// The run-time A/B switches of the library: one table (tuning.hip) holds every roma_tuning key and every integer ROMA_*
// environment variable with its default.  A call site asks for the value and keeps whatever it derives from it.
#pragma once
#include <string>

namespace roma {

enum Switch : int {
  SW_GEMM8P,
  SW_GEMM_DBG,
  SW_GEMM8P_WALK,
  SW_GEMM8P_SCHED,
  SW_GEMM8P_MAXWG,
  SW_WS1X1,
  SW_LC_MODE,
  SW_LC_BIN,
  SW_CONV64,
  SW_CONV_PATCH,
  SW_ATTN_XCD,
  SW_ATTN_EXP2,
  SW_DW_RING,
  SW_GP_COL,
  SW_POOL_PROJ,
  SW_GP_COL_LEADER,
  SW_GEMM8P_MINM,
  SW_GEMM_NT,
  SW_GEMM_F32_FILL,
  SW_GEMM_SMALLM,
  SW_CONV64_SY,
  SW_CONV_KORDER,
  SW_RB_SY,
  SW_DWR_MAXSY,
  SW_DW_RING_MINELEMS,
  SW_RI_VEC,
  SW_OUT_ROW,
  SW_OUT_LPR,
  SW_OUT_ROWS_IT,
  SW_GP_AUG,
  SW_GP_BWD2,
  SW_COMPOSE_OUT,
  SW_VIT_RES_F32,
  SW_STREAMS,
  SW_STREAMS_SERIAL,
  SW_DEBUG_DUAL_SLOT,
  SW_COUNT
};

// The effective value: the roma_tuning override if one is set at or above the row's lowest override value, else the
// environment (parsed once per process, at the first use of the table), else the default.  An array index and the guard of
// one function-local static; safe to call while other translation units are still in static initialisation.
long tuning(Switch id);
// The two halves on their own, for the few sites that consult only one: environment value or default (what holds with no
// override), and the override alone (-1 when none is set).
long tuning_env(Switch id);
long tuning_override(Switch id);
// Behind roma_tuning: 0, or ROMA_ERR_ARG with "roma_tuning: unknown key <key>".  A value below the row's lowest override
// value clears the override.  Like the launches that read them, overrides are not synchronised: set them between launches.
int tuning_set(const char* key, long value);
// Behind roma_tuning_describe: a JSON array, one object per row in table order.
std::string tuning_describe();

}  // namespace roma
