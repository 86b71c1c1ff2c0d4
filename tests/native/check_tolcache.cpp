// tfp_tolcache.hpp (the engine's per-(tolerance, version) caches) on the CPU, with a counting dummy
// payload: a "build" is a claim + commit, as the engine's ensure_* functions do it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "../../asterisk-tiresias_amd/csrc/tfp_tolcache.hpp"

struct Payload {
  int id;           // which payload object this is (buffer reuse: a claim hands out the victim's)
  int builds = 0;   // builds into this object
  double built_for = -1;
  static int made;
  Payload() : id(made++) {}
};
int Payload::made = 0;

using Cache = tfp::TolCache<Payload, 4>;  // 1 active + 3, as both of the engine's LRUs
static long n_builds = 0, n_checks = 0;

#define CHECK(x)                                                 \
  do {                                                           \
    n_checks++;                                                  \
    if (!(x)) {                                                  \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);        \
      exit(1);                                                   \
    }                                                            \
  } while (0)

// the engine's lookup: the committed entry, or a build into a claimed one
static Payload* get(Cache& c, double tol, uint64_t v, bool commit = true) {
  if (Payload* p = c.find(tol, v)) return p;
  Payload* p = c.claim(v);
  n_builds++;
  p->builds++;
  p->built_for = tol;
  if (commit) c.commit(tol, v);
  return p;
}

int main() {
  const double T[5] = {0.001, 0.01, 0.1, 0.45, 0.3};
  {  // four tolerances, 1 + 3 entries: each built once, then any alternation builds nothing
    Cache c;
    for (int i = 0; i < 4; i++) get(c, T[i], 1);
    CHECK(n_builds == 4 && Payload::made == 4);
    unsigned x = 12345;
    for (int i = 0; i < 1000; i++) {
      x = x * 1664525u + 1013904223u;
      const double t = T[(x >> 16) % 4];
      CHECK(get(c, t, 1)->built_for == t);
    }
    CHECK(n_builds == 4);
    // a fifth evicts exactly the one least recently active: make the order 0, 2, 1, 3 (3 active)
    for (int i : {0, 2, 1, 3}) get(c, T[i], 1);
    Payload* lru = c.find(T[0], 1);
    for (int i : {2, 1, 3}) get(c, T[i], 1);  // T[0] stopped being active first again
    CHECK(n_builds == 4);
    Payload* p5 = get(c, T[4], 1);
    CHECK(n_builds == 5 && p5 == lru && p5->builds == 2);  // the victim's payload object, not a fresh one
    for (int i : {4, 1, 2, 3, 4, 3}) get(c, T[i], 1);
    CHECK(n_builds == 5);                                   // the other three and the fifth are hits
    CHECK(c.find(T[0], 1) == nullptr);                      // ... and the evicted one is gone
    // while the active entry is valid, claim never picks it (whatever its age)
    Payload* act = c.find(T[3], 1);
    for (int i = 0; i < 8; i++) {
      CHECK(c.claim(1) != act);
      c.commit(10.0 + i, 1);
      act = &c.active();
    }
  }
  {  // a version bump expires every entry except a carried active one
    Cache c;
    for (int i = 0; i < 4; i++) get(c, T[i], 1);
    Payload* a = c.find(T[2], 1);
    c.carry(2);
    CHECK(c.find(T[2], 2) == a && c.find(T[2], 1) == nullptr);
    for (int i : {0, 1, 3}) CHECK(c.find(T[i], 2) == nullptr);
    CHECK(c.find(T[2], 2) == a && &c.active() == a);
    const long b0 = n_builds;
    get(c, T[0], 2);  // (the claim at version 2 expires the version-1 entries for good)
    CHECK(n_builds == b0 + 1 && c.find(T[1], 1) == nullptr && c.find(T[3], 1) == nullptr && c.find(T[2], 2) == a);
    c.invalidate_active();
    CHECK(c.find(T[2], 2) == nullptr && !c.active_valid());
    c.carry(3);  // (nothing valid to carry)
    CHECK(c.find(T[2], 3) == nullptr);
  }
  {  // claim without commit: no find serves the entry at any tolerance, the one it held included
    Cache c;  // ... when the claimed entry was a valid LRU victim
    for (int i = 0; i < 4; i++) get(c, T[i], 1);
    Payload* victim = c.find(T[0], 1);
    for (int i : {1, 2, 3}) get(c, T[i], 1);
    Payload* p = get(c, T[4], 1, /*commit=*/false);
    CHECK(p == victim);
    for (double t : {T[0], T[4], 0.0}) CHECK(c.find(t, 1) == nullptr);
    for (int i : {1, 2, 3}) CHECK(c.find(T[i], 1) != nullptr && c.find(T[i], 1) != p);
    CHECK(get(c, T[4], 1) == p && c.find(T[4], 1) == p);  // the next build reuses it, and commits
    Cache d;  // ... and when it was an expired one
    for (int i = 0; i < 4; i++) get(d, T[i], 1);
    Payload* q = get(d, T[1], 2, /*commit=*/false);
    for (uint64_t v = 1; v <= 2; v++)
      for (int i = 0; i < 5; i++) CHECK(d.find(T[i], v) != q);
    CHECK(d.find(T[1], 2) == nullptr && !d.active_valid() && &d.active() == q);
  }
  {  // tolerances compare bitwise
    Cache c;
    const long b0 = n_builds;
    Payload* pz = get(c, 0.0, 1);
    Payload* nz = get(c, -0.0, 1);
    CHECK(pz != nz && n_builds == b0 + 2 && c.find(0.0, 1) == pz && c.find(-0.0, 1) == nz);
    const double nan = std::nan("");
    Payload* pn = get(c, nan, 1);
    CHECK(c.find(nan, 1) == pn && get(c, nan, 1) == pn && n_builds == b0 + 3);
  }
  {  // the single entry (the delta's cache, the key boxes)
    tfp::TolEntry<Payload> e;
    CHECK(!e.holds(0.5, 1));
    Payload* p = e.begin();
    CHECK(p == &e.p && !e.holds(0.5, 1));
    e.commit(0.5, 1);
    CHECK(e.holds(0.5, 1) && !e.holds(0.5, 2) && !e.holds(0.25, 1));
    e.carry(2);
    CHECK(e.holds(0.5, 2) && !e.holds(0.5, 1));
    e.begin();
    CHECK(!e.holds(0.5, 2));
    e.carry(3);
    CHECK(!e.holds(0.5, 3));
  }
  printf("tolcache: %ld checks, %d payload objects\nOK\n", n_checks, Payload::made);
  return 0;
}
