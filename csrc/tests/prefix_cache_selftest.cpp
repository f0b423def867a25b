// Randomised self-test of the scheduler's prefix cache (csrc/runtime/runtime_core.h), built with
// AddressSanitizer + UndefinedBehaviorSanitizer and, separately, the libstdc++ debug checks by
// tests/test_prefix_cache_sanitizers.py (host code only).  Exits non-zero on the first broken invariant.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#include "../runtime/runtime_core.h"

#define REQUIRE(c)                                                       \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: invariant failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

template <typename F>
static bool throws(F f) {
  try {
    f();
  } catch (const std::exception&) {
    return true;
  }
  return false;
}

// prompts that share prefixes of every length: a cut of one of three base sequences, then a private tail
static std::vector<int> prompt(std::mt19937& rng, int n) {
  const int base = rng() % 3, cut = rng() % (n + 1), salt = 4 + rng() % 5;
  std::vector<int> t(n);
  for (int i = 0; i < n; ++i) t[i] = i < cut ? (7 * i + 13 * base * (i + 1)) % 251 : (5 * i + 11 * salt * (i + 3)) % 241;
  return t;
}

static void check(const Scheduler& s, int blocks) {
  const auto nodes = s.prefix_nodes();
  std::map<int, long long> refs;
  int evictable = 0;
  for (const auto& n : nodes) {
    REQUIRE(n[0] >= 1 && n[0] < blocks && refs.emplace((int)n[0], n[1]).second);
    REQUIRE(n[1] >= 0);
    evictable += n[1] == 0;
  }
  std::map<int, long long> holders;
  std::set<int> priv;
  for (long long id : s.running()) {
    const auto t = s.block_table(id);
    const int k = s.shared_blocks(id);
    REQUIRE(k >= 0 && k <= (int)t.size());
    REQUIRE(s.cached_tokens(id) >= 0);
    for (int i = 0; i < (int)t.size(); ++i) {
      REQUIRE(t[i] >= 1 && t[i] < blocks);
      if (i < k) {
        REQUIRE(refs.count(t[i]));
        ++holders[t[i]];
      } else {
        REQUIRE(!refs.count(t[i]) && priv.insert(t[i]).second);
      }
    }
  }
  for (const auto& n : nodes) REQUIRE(n[1] >= holders[(int)n[0]]);  // pins of pending copies come on top
  REQUIRE(s.cached_blocks() == (int)nodes.size());
  REQUIRE(s.free_blocks() - evictable + (int)priv.size() + (int)nodes.size() == blocks - 1);
  REQUIRE(s.kv_usage() >= -1e-12 && s.kv_usage() <= 1.0 + 1e-12);
}

static void drive(std::mt19937& rng, int cow_min, int steps) {
  const int blocks = 33, bs = 64, slots = 6, maxb = 12;
  Scheduler s(blocks, bs, slots, 600, maxb, 64, true, cow_min);
  long long next = 1;
  std::map<long long, std::pair<std::vector<int>, int>> known;  // id -> prompt, max_new
  bool pending = false;
  for (int step = 0; step < steps; ++step) {
    const int op = rng() % 8;
    if (op == 0 || op == 1) {
      const int n = 1 + rng() % 500, m = 1 + rng() % 300;
      const auto p = prompt(rng, n);
      const bool cacheable = rng() % 8 != 0;
      if ((n + m + bs - 1) / bs > maxb) {
        REQUIRE(throws([&] { s.add(next, n, m, p, cacheable); }));
      } else {
        if (cacheable) REQUIRE(throws([&] { s.add(next, n, m, std::vector<int>(p.begin(), p.end() - 1)); }));
        s.add(next, n, m, p, cacheable);
        known[next] = {p, m};
      }
      ++next;
    } else if (op == 2) {
      for (long long id : s.admit()) {
        const auto& p = known.at(id).first;
        REQUIRE(s.cached_tokens(id) <= (int)p.size() - 1);
        REQUIRE(s.shared_blocks(id) * bs <= s.cached_tokens(id) && s.cached_tokens(id) < (s.shared_blocks(id) + 1) * bs);
        pending = true;
      }
      if (rng() % 4) {  // mostly as the engine does: copies taken and acknowledged right after admit()
        std::set<int> dsts;
        for (const auto& c : s.take_copies()) {
          REQUIRE(c.first != c.second && c.first >= 1 && c.second >= 1 && dsts.insert(c.second).second);
          bool cached_src = false;
          for (const auto& n : s.prefix_nodes()) cached_src |= n[0] == c.first && n[1] >= 1;
          REQUIRE(cached_src);  // still in the index, and pinned
        }
        s.copies_done();
        pending = false;
      }
    } else if (op == 3 && s.num_running() > 0) {
      const auto run = s.running();
      s.publish(run[rng() % run.size()]);
    } else if (op == 4 && s.num_running() > 0) {
      const auto run = s.running();
      const long long id = run[rng() % run.size()];
      const int before = (int)s.block_table(id).size();
      const int got = s.grow(id, 1 + rng() % (bs * maxb + 100));
      REQUIRE((int)s.block_table(id).size() == before + std::max(got, 0) && (int)s.block_table(id).size() <= maxb);
    } else if (op == 5 && s.num_running() > 0) {
      const long long id = s.youngest_first().front();
      auto& k = known.at(id);
      std::vector<int> p = k.first;
      for (int i = rng() % 40; i > 0; --i) p.push_back(rng() % 200);
      const int m = std::max(1, k.second - (int)(p.size() - k.first.size()));
      if (((int)p.size() + m + bs - 1) / bs > maxb) {
        REQUIRE(throws([&] { s.preempt(id, (int)p.size(), m, p); }));
      } else {
        s.preempt(id, (int)p.size(), m, p);
        REQUIRE(s.slot(id) == -1 && s.block_table(id).empty() && s.cached_tokens(id) == 0);
        k = {p, m};
      }
    } else if (op == 6 && !known.empty()) {
      auto it = known.begin();
      std::advance(it, rng() % known.size());
      s.finish(it->first);
      known.erase(it);
    } else if (op == 7 && rng() % 8 == 0) {
      s.reset_prefix_cache();
      if (!pending) {
        for (const auto& n : s.prefix_nodes()) REQUIRE(n[1] > 0);
      }
    }
    check(s, blocks);
  }
  for (const auto& k : known) s.finish(k.first);
  s.copies_done();
  s.reset_prefix_cache();
  REQUIRE(s.cached_blocks() == 0 && s.free_blocks() == blocks - 1 && s.num_running() == 0 && s.num_waiting() == 0);
}

int main() {
  std::mt19937 rng(4321);
  for (int cow_min : {1, 16, 64}) drive(rng, cow_min, 4000);
  std::puts("prefix cache selftest ok");
  return 0;
}
