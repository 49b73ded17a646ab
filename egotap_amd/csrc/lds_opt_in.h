// Which (kernel, device) pairs have been allowed how many bytes of dynamic LDS: the bookkeeping behind ego_allow_dynamic_lds (common.h).
// No HIP here -- the call that raises the limit is the caller's `set` -- so a CPU program can exercise it (tests/lds_opt_in_main.cpp).
#pragma once
#include <map>
#include <mutex>
#include <utility>

class LdsOptIn {
  public:
    // Runs set(bytes) unless the pair already holds at least `bytes`, and records the new size when set returns success (a value-
    // initialised result: hipSuccess).  A failure is returned and not recorded: the next launch tries again.  The lock is held across
    // set, so a second thread asking for the same pair returns only after the limit is raised, never between the record and the call.
    template <class Set>
    auto ensure(const void* kernel, int device, int bytes, Set&& set) -> decltype(set(bytes)) {
        using R = decltype(set(bytes));
        std::lock_guard<std::mutex> lock(mu_);
        int& have = bytes_[{kernel, device}];      // 0 when new: the default limit needs no call
        if (bytes <= have) return R{};
        const R r = set(bytes);
        if (r == R{}) have = bytes;
        return r;
    }

  private:
    std::mutex mu_;
    std::map<std::pair<const void*, int>, int> bytes_;
};
