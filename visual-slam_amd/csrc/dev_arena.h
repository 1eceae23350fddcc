// The device memory of a solve, stated once: ba.hip, ba_fused.hip and pgo.hip collect their buffers in an ArenaPlan,
// make ONE allocation for all of them (40 hipMalloc calls cost more than 3 LM iterations of a local window) and get
// typed pointers into it.  The plan is plain C++ (tests/cpp/dev_arena_test.cpp drives it on the CPU); the DevArena that
// holds the block needs HIP.  Offsets follow request order -- the relative placement of S, F, E, Wg and Yg decides which
// HBM channels they fall on, so the order of the add() calls of a solver is part of its tuning.
#pragma once
#include <cassert>
#include <cstddef>
#include <cstring>
#include <vector>

// a buffer's share of a block: at least 8 bytes (an empty buffer still gets an address of its own), in 256-byte steps
inline size_t arena_slot(size_t bytes) { return ((bytes > 8 ? bytes : 8) + 255) & ~(size_t)255; }

class ArenaPlan {
  struct Req { void* where; size_t offset; };  // where: address of the caller's T*
  std::vector<Req> reqs_;
  size_t total_ = 0;

 public:
  explicit ArenaPlan(size_t expected_requests = 0) { reqs_.reserve(expected_requests); }
  // `where` is assigned by bind() and has to live until then
  template <class T>
  void add(T*& where, size_t count) {
    reqs_.push_back({&where, total_});
    total_ += arena_slot(sizeof(T) * count);
  }
  size_t total() const { return total_; }
  void bind(void* base) const {
    for (const Req& r : reqs_) {
      char* at = (char*)base + r.offset;
      memcpy(r.where, &at, sizeof(at));  // (every T* here is an object pointer: one representation)
    }
  }
};

#if defined(__HIPCC__)
#include "vsl_common.h"

// Who pays for the block.  OWNED: hipMalloc here, hipFree with the DevArena (sessions, the parity hooks, the pose graph).
// BORROWED: the context's cached arena, grown to total + total / 4 when it is too small and marked busy until the
// DevArena dies (vsl_bundle_adjust, on both of its paths: one allocation reused across the solves of a context); when
// that arena is lent out already, a private block as under OWNED.
enum class ArenaPolicy { OWNED, BORROWED };

class DevArena {
  void* own_ = nullptr;        // freed here
  vsl_ctx* lender_ = nullptr;  // whose ba_arena_busy to clear
 public:
  DevArena() = default;
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() {
    if (own_) (void)hipFree(own_);
    if (lender_) lender_->ba_arena_busy = false;
  }
  // one block for the plan, every requested pointer set; call once per DevArena
  hipError_t acquire(vsl_ctx* ctx, ArenaPolicy policy, const ArenaPlan& plan) {
    assert(!own_ && !lender_);
    const size_t total = plan.total();
    hipError_t e;
    if (policy == ArenaPolicy::OWNED || ctx->ba_arena_busy) {
      if ((e = hipMalloc(&own_, total)) != hipSuccess) return e;
      plan.bind(own_);
      return hipSuccess;
    }
    if (ctx->ba_arena_cap < total) {
      if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return e;
      if (ctx->ba_arena) (void)hipFree(ctx->ba_arena);
      ctx->ba_arena = nullptr;
      ctx->ba_arena_cap = 0;
      const size_t cap = total + total / 4;
      if ((e = hipMalloc(&ctx->ba_arena, cap)) != hipSuccess) return e;
      ctx->ba_arena_cap = cap;
    }
    ctx->ba_arena_busy = true;
    lender_ = ctx;
    plan.bind(ctx->ba_arena);
    return hipSuccess;
  }
};
#endif
