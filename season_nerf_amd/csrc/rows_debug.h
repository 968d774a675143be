// Test introspection of the row GEMMs' routing (include/season_nerf_hip.h: snerf_rows_debug_set, snerf_rows_record_reset / _read).  Host code only.
//   per thread:   an override of the RowsSwitches (every reader of rows_switches() sees it), a dry-run bit (a routed product is planned and recorded,
//                 nothing is launched, no pointer is dereferenced) and an x_padded bit (the public snerf_linear_* calls set Product::x_padded);
//   per process:  the set of distinct plans executed or dry-run since the last reset (the training engine's backward runs on another thread than its
//                 caller, so the record and its on/off bit cannot be per thread).
// What the default path pays: one test of `tl_rows_debug.active` and one relaxed load of `rows_record_on` per product.
#pragma once
#include <atomic>
#include <stdint.h>

namespace snerf {

struct RowsDebug { bool active, override_sw, dry_run, x_padded; };      // active: any of the three others is set
inline thread_local RowsDebug tl_rows_debug = {false, false, false, false};
inline std::atomic<bool> rows_record_on{false};

// One entry of the record, as snerf_rows_record_read hands it out: route (0 Thin, 1 Rows, 2 Fp32 - linear_product.h Route), then - Rows only, else
// kernel = -1 and the rest 0 - RowsPlan's kernel (RowsKernel), nt, pf, aol, act, hv, tab_lds, zero_bn, split (SplitLayout), grid, LDS bytes.
constexpr int ROWS_RECORD_INTS = 12;

// the weight-gradient launches of the calling thread since wgrad_note_begin (snerf_train_kernel_debug "wgrad"): per launch kernel | partial << 6 | reverse << 7
struct WgradNote { bool on; int n; int v[2]; };
inline thread_local WgradNote tl_wgrad_note = {false, 0, {0, 0}};
inline void wgrad_note_begin() { tl_wgrad_note = WgradNote{true, 0, {0, 0}}; }
inline void wgrad_note_plan(int packed) { if (tl_wgrad_note.on && tl_wgrad_note.n < 2) tl_wgrad_note.v[tl_wgrad_note.n++] = packed; }
inline int wgrad_note_end() { tl_wgrad_note.on = false; return tl_wgrad_note.n == 0 ? -1 : tl_wgrad_note.v[0] | (tl_wgrad_note.n > 1 ? tl_wgrad_note.v[1] << 8 : 0); }

inline bool rows_dry_run() { return tl_rows_debug.active && tl_rows_debug.dry_run; }
inline bool rows_x_padded() { return tl_rows_debug.active && tl_rows_debug.x_padded; }
inline bool rows_noting() { return rows_record_on.load(std::memory_order_relaxed) || rows_dry_run(); }

// gemm.hip
void rows_debug_set(const int* switches8, bool dry_run, bool x_padded);      // switches8: the RowsSwitches fields in their order, or NULL = the process's own
void rows_record_reset(bool on);                                             // empties the record; on: record from now on
int rows_record_read(int32_t* out, int max_entries);                         // returns the number of entries the record holds; copies at most max_entries
void rows_note_route(int route);                                             // a product on the Thin (0) or Fp32 (2) route (a Rows plan: launch_gemm_bf16x3)

}  // namespace snerf
