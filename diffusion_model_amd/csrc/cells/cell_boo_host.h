// Host-only argument validation of the bond-orientational-order entries (cell_boo.hip) and of their host statement.  Plain C++
// beside host_logic: it is also compiled into the CPU-only sanitizer library (make asan).
#pragma once
#include "cell_soap_host.h"

namespace egnn {

// every check returns EGNN_OK or EGNN_EINVAL with the message set; nothing is launched before they pass.
// A, l_max and l_solid (-1: the entry reads none) in range, select within its A x A bits
int cell_boo_config_check(const char* who, int A, int l_max, int l_solid, unsigned select);
// g_off a HOST array of l_max + 2 offsets: from 0, not decreasing, ending at E
int cell_boo_table_check(const char* who, int l_max, int E, const int32_t* g_off);

}  // namespace egnn
