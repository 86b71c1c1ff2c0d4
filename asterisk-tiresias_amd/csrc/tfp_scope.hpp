// tfp_scope.hpp — context-scoped search: the first K rows of the reference's result query
// (fp_handler.c:367-374) when the per-frame insert (:308-314) also carries "and context = '<s>'",
// which its documentation promises (doc/dialplan_application.rst:11, :52-53) and its SQL omits.
// A clip carries a scope (int32 >= 0, 0 when new); a query names one, or kScopeAny for every clip.
// The rows are ranked search's (tfp_rank.hpp) over the scope's clips alone: a column out of scope
// has key 0, inside the kernels, so a wanted clip below the global first K rows is still found.
//
// The per-column scope table: one int32 per index column (main columns, then the delta's after
// them), kScopeNone where a column holds no clip, padded to a multiple of 4 columns so a thread of
// the vote form reads its four columns' scopes as one 16-byte load.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_kernels.hpp"
#include "tfp_rank.hpp"

namespace tfp {

constexpr int32_t kScopeAny = -1;   // TFP_SCOPE_ANY: a query over every clip
constexpr int32_t kScopeNone = -2;  // a column without a clip: in no scope (ANY is bounded by C)
inline int32_t scope_table_cols(int32_t C) { return (C + 3) / 4 * 4; }

// d_table[c] = the scope of column c's clip for c < scope_table_cols(C): d_clip_scope[d_col_clip[c]],
// or kScopeNone where d_col_clip[c] < 0. d_col_clip holds scope_table_cols(C) entries.
hipError_t launch_scope_table(const int32_t* d_col_clip, const int32_t* d_clip_scope, int32_t C, int32_t* d_table,
                              hipStream_t s);

// launch_rank_vote with a scope per query (d_qscope[q], >= kScopeAny) over the table d_table; the
// other arguments, the scratch and *d_bad as there.
hipError_t launch_scope_vote(const double* d_q, const int64_t* d_qoff, const int32_t* d_qscope, int32_t nq, SearchConsts sc,
                             const uint32_t* d_bits, int32_t C, const int32_t* d_tiekey, const int32_t* d_table, int32_t K,
                             unsigned long long* d_part, unsigned long long* d_keys, int32_t* d_bad, hipStream_t s);

// The general form's selection after launch_scan_touched (tfp_kernels.hpp) counted queries
// [q_begin, q_begin + nq): d_keys[(q_begin + q) * K + r] = the r-th greatest key among the query's
// touched clips in scope d_qscope[q_begin + q]; the scratch of every touched clip, in scope or not,
// restored to zero.
hipError_t launch_scope_final(int32_t q_begin, int32_t nq, const int32_t* d_qscope, const int32_t* d_tiekey,
                              const int32_t* d_table, int32_t C, int32_t* d_stamp, int32_t* d_score,
                              const int32_t* d_touched, int32_t* d_tcnt, int32_t K, unsigned long long* d_keys,
                              hipStream_t s);

}  // namespace tfp
