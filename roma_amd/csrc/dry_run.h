// Private to the host-side schedules (model.hip, gp.hip): a planning (dry) run walks the same code and skips every launch.
#pragma once

#define RUN(expr)                 \
  do {                            \
    if (!dry) {                   \
      int _rc = (expr);           \
      if (_rc) return _rc;        \
    }                             \
  } while (0)
