// What msm.hip calls in msm_tables.hip (the table preparation, instantiated there per curve).
#pragma once
#include "ctx.hpp"

namespace vk {
struct GlvK;  // msm_digits.hpp
GlvK glv_consts();
int glv_table_ok(vc_ctx* ctx, Table* t, bool* ok);
template <class C>
int fast_tables(vc_ctx* ctx, Table* t, bool with_phi);
template <class C>
int win_tables(vc_ctx* ctx, Table* t, int c, int W, int ts, uint32_t mul = 1, bool pair = false);
}  // namespace vk
