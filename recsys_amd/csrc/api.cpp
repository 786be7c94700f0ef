// Version / error strings of librsx.so.
#include "rsx.h"

extern "C" int rsx_version(void) { return 107; /* 0.1.7: rsx_rows_dot, rsx_topk_rows_counted, rsx_din_retrieve_candidates; 106: rsx_topk_rows_rules; 105: rsx_rank_count_rows; 104: rsx_predict_din_rank_shared, rsx_topk_rows_excl, rsx_topk_rows_threads; 103: the device parse of TFRecord records (rsx_criteo_parse_records); 102: the device parse entries (rsx_criteo_parse_examples, rsx_log_thresholds_h); 101: table_dtype appended to the predict models */ }

extern "C" const char* rsx_strerror(int status) {
  switch (status) {
    case RSX_OK: return "ok";
    case RSX_EINVAL: return "invalid argument";
    case RSX_ELAUNCH: return "kernel launch failed (hipGetLastError)";
    case RSX_EUNSUPPORTED: return "request outside the implemented envelope";
    case RSX_EDATA: return "corrupt input data";
    case RSX_ECOMM: return "collective library call failed (see rsx_comm_last_error_h)";
    default: return "unknown rsx status";
  }
}

#include "rsx_launch_count.h"
extern "C" unsigned long long rsx_dbg_launch_count(void) { return rsx_launches_g.load(std::memory_order_relaxed); }
