/* Layout of the structures that roma_amd/_lib.py restates as ctypes structures: compiled as C99 (which also holds
 * include/roma_hip.h to being a C header) and run by tests/test_cpu_abi.py.  One line per fact: struct, field ("sizeof" for
 * the size of the whole), bytes. */
#include <stddef.h>
#include <stdio.h>

#include "roma_hip.h"

#define SIZE(T) printf(#T " sizeof %zu\n", sizeof(T))
#define FIELD(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))

int main(void) {
  SIZE(roma_config_t);
  FIELD(roma_config_t, coarse_h);
  FIELD(roma_config_t, coarse_w);
  FIELD(roma_config_t, upsample_h);
  FIELD(roma_config_t, upsample_w);
  FIELD(roma_config_t, symmetric);
  FIELD(roma_config_t, upsample_preds);
  FIELD(roma_config_t, attenuate_cert);
  FIELD(roma_config_t, precision);
  FIELD(roma_config_t, max_batch);
  FIELD(roma_config_t, device);
  SIZE(roma_forward_args_t);
  FIELD(roma_forward_args_t, upsample);
  FIELD(roma_forward_args_t, symmetric);
  FIELD(roma_forward_args_t, scale_factor);
  FIELD(roma_forward_args_t, seed_flow);
  FIELD(roma_forward_args_t, seed_cert);
  FIELD(roma_forward_args_t, seed_h);
  FIELD(roma_forward_args_t, seed_w);
  FIELD(roma_forward_args_t, flow);
  FIELD(roma_forward_args_t, cert);
  FIELD(roma_forward_args_t, feat);
  return 0;
}
