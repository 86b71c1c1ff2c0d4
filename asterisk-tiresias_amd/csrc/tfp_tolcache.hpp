// tfp_tolcache.hpp — a payload cached per (tolerance, version): the engine's search-side caches
// (csrc/tfp_engine.cpp). The dialplan passes the tolerance per call (application_handler.c:114-122),
// so extensions at different tolerances alternate on one engine; the version is the index's.
// Host-only (no HIP call, no engine type) so tests/native/check_tolcache.cpp drives it on the CPU.
//
// One discipline for every cache: a payload is served only between commit() and the next begin() /
// claim() / version change. A build that returns early leaves its entry uncommitted, and no later
// lookup can take it for a cache of any tolerance.
#pragma once

#include <stdint.h>
#include <string.h>

namespace tfp {

// One payload and the (tolerance, version) it was committed at. Tolerances compare bitwise.
template <class P>
class TolEntry {
 public:
  P p;
  bool valid() const { return valid_; }
  bool holds(double tol, uint64_t version) const {
    return valid_ && version_ == version && memcmp(&tol_, &tol, sizeof tol) == 0;
  }
  double tol() const { return tol_; }
  // the payload handed to a build (its buffers reused), served again only after commit()
  P* begin() {
    valid_ = false;
    return &p;
  }
  void commit(double tol, uint64_t version) {
    tol_ = tol;
    version_ = version;
    valid_ = true;
  }
  // the payload was brought up to the index at new_version (or does not depend on the change)
  void carry(uint64_t new_version) {
    if (valid_) version_ = new_version;
  }
  void invalidate() { valid_ = false; }
  void expire(uint64_t version) { valid_ = valid_ && version_ == version; }

 private:
  double tol_ = 0.0;
  uint64_t version_ = 0;
  bool valid_ = false;
};

// N entries, one of them active (the one the engine works on), the others least recently active
// first out. Switching the active entry is an index change: no payload moves.
template <class P, int N>
class TolCache {
  static_assert(N >= 2, "one active entry and at least one beside it (a single entry: TolEntry)");

 public:
  // The committed entry of (tol, version), made active; nullptr when there is none.
  P* find(double tol, uint64_t version) {
    for (int i = 0; i < N; i++)
      if (e_[i].holds(tol, version)) return activate(i);
    return nullptr;
  }
  // A miss: the entry to build into, active and invalid until commit(). An invalid or expired one
  // (the active one first: its buffers are the warmest), else the valid one that stopped being
  // active longest ago; never the active entry while it is valid.
  P* claim(uint64_t version) {
    for (auto& t : e_) t.expire(version);
    int v = e_[act_].valid() ? -1 : act_;
    for (int i = 0; i < N && e_[act_].valid(); i++) {
      if (i == act_) continue;
      if (v < 0 || (e_[i].valid() != e_[v].valid() ? !e_[i].valid() : used_[i] < used_[v])) v = i;
    }
    e_[v].begin();
    return activate(v);
  }
  void commit(double tol, uint64_t version) { e_[act_].commit(tol, version); }
  void carry(uint64_t new_version) { e_[act_].carry(new_version); }
  void invalidate_active() { e_[act_].invalidate(); }
  bool active_valid() const { return e_[act_].valid(); }
  double active_tol() const { return e_[act_].tol(); }
  P& active() { return e_[act_].p; }

 private:
  P* activate(int i) {
    if (i != act_) used_[act_] = ++clock_;  // (stamped when it stops being active)
    act_ = i;
    return &e_[i].p;
  }
  TolEntry<P> e_[N];
  uint64_t used_[N] = {};
  uint64_t clock_ = 0;
  int act_ = 0;
};

}  // namespace tfp
