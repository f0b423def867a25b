// Randomised self-test of the scheduler's context shift (csrc/runtime/runtime_core.h Scheduler::shift) next to the
// prefix cache: a fuzz of add / admit / publish / grow / shift / preempt / finish, built with AddressSanitizer +
// UndefinedBehaviorSanitizer and, separately, the libstdc++ debug checks by tests/test_context_shift_sanitizers.py
// (host code only).  Exits non-zero on the first broken invariant.
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

// prompts that share prefixes of every length: a cut of one of two base sequences, then a private tail
static std::vector<int> prompt(std::mt19937& rng, int n) {
  const int base = rng() % 2, cut = rng() % (n + 1), salt = 4 + rng() % 5;
  std::vector<int> t(n);
  for (int i = 0; i < n; ++i) t[i] = i < cut ? (7 * i + 13 * base * (i + 1)) % 251 : (5 * i + 11 * salt * (i + 3)) % 241;
  return t;
}

// No block is owned twice, shared heads are chains from the root (a holder holds every ancestor, and the index
// counts it), and every block is accounted for: free + evictable, private, cached, or held for a pending shift.
static void check(const Scheduler& s, int blocks) {
  const auto nodes = s.prefix_nodes();
  std::map<int, long long> refs, parent;
  int evictable = 0;
  for (const auto& n : nodes) {
    REQUIRE(n[0] >= 1 && n[0] < blocks && refs.emplace((int)n[0], n[1]).second);
    REQUIRE(n[1] >= 0);
    parent[(int)n[0]] = n[4];
    evictable += n[1] == 0;
  }
  std::map<int, long long> holders;
  std::set<int> priv;
  for (long long id : s.running()) {
    const auto t = s.block_table(id);
    const int k = s.shared_blocks(id);
    REQUIRE(k >= 0 && k <= (int)t.size());
    for (int i = 0; i < (int)t.size(); ++i) {
      REQUIRE(t[i] >= 1 && t[i] < blocks);
      if (i < k) {
        REQUIRE(refs.count(t[i]));
        REQUIRE(parent.at(t[i]) == (i ? t[i - 1] : -1));  // the chain: every ancestor is in the request's own head
        ++holders[t[i]];
      } else {
        REQUIRE(!refs.count(t[i]) && priv.insert(t[i]).second);
      }
    }
  }
  for (const auto& n : nodes) {
    REQUIRE(n[1] >= holders[(int)n[0]]);  // pins of pending copies and shifts come on top
    if (n[4] >= 0) REQUIRE(refs.at((int)n[4]) >= n[1]);  // whoever holds a node holds its parent
  }
  REQUIRE(s.cached_blocks() == (int)nodes.size());
  REQUIRE(s.free_blocks() - evictable + (int)priv.size() + (int)nodes.size() + s.shift_held_blocks() == blocks - 1);
}

// One shift of a running request, checked against the rule: the table below keep / bs is untouched, every entry from
// there on is the old entry d / bs further up when the request owned it and a fresh block otherwise, the moves cover
// every row of the new blocks exactly once, no destination is held by the index, and a refusal changes nothing.
static void shift_one(Scheduler& s, std::mt19937& rng, long long id, int blocks, int bs) {
  const auto old = s.block_table(id);
  const int nb = (int)old.size(), shared = s.shared_blocks(id), free_before = s.free_blocks();
  const int held_before = s.shift_held_blocks();  // of an earlier shift whose moves are not acknowledged yet
  const int keep = (rng() % 3 == 0) ? 0 : (int)(rng() % (bs * 2 + 7));
  const int m = 1 + rng() % 3, d = m * bs, k0 = keep / bs, rem = keep % bs;
  REQUIRE(throws([&] { s.shift(id, keep, d + 1); }));
  REQUIRE(throws([&] { s.shift(id, -1, d); }));
  REQUIRE(throws([&] { s.shift(id, keep, 0); }));
  if (k0 + m >= nb) {
    REQUIRE(throws([&] { s.shift(id, keep, d); }));
    REQUIRE(s.block_table(id) == old);
    return;
  }
  const Scheduler::ShiftPlan p = s.shift(id, keep, d);
  std::set<int> indexed;  // as the index stands now: taking the fresh blocks may have evicted unreferenced nodes
  for (const auto& n : s.prefix_nodes()) indexed.insert((int)n[0]);
  if (!p.ok) {  // the shared tail needed more fresh blocks than the arena has
    REQUIRE(s.block_table(id) == old && s.shared_blocks(id) == shared && s.free_blocks() == free_before);
    REQUIRE(p.moves.empty() && p.table.empty() && s.shift_held_blocks() == held_before);
    return;
  }
  const auto now = s.block_table(id);
  REQUIRE(now == p.table && (int)now.size() == nb - m && s.shared_blocks(id) == std::min(shared, k0));
  std::set<int> olds(old.begin(), old.end());
  std::map<int, std::vector<int>> rows;  // dst -> times each row is written
  for (int j = 0; j < nb - m; ++j) {
    if (j < k0) {
      REQUIRE(now[j] == old[j]);
    } else if (j + m >= shared) {
      REQUIRE(now[j] == old[j + m]);  // in place
    } else {
      REQUIRE(!olds.count(now[j]));   // fresh
    }
    if (j >= k0) REQUIRE(!indexed.count(now[j]));
  }
  for (const auto& mv : p.moves) {
    REQUIRE(mv.size() == 5 && mv[2] >= 0 && mv[2] < mv[3] && mv[3] <= bs);
    REQUIRE(mv[0] >= 1 && mv[0] < blocks && mv[1] >= 1 && mv[1] < blocks && !indexed.count(mv[1]));
    const auto it = std::find(now.begin() + k0, now.end(), mv[1]);
    REQUIRE(it != now.end());
    const int j = (int)(it - now.begin());
    if (mv[4] == 0) {
      REQUIRE(j == k0 && rem && mv[0] == old[k0] && mv[2] == 0 && mv[3] == rem);
    } else {
      REQUIRE(mv[4] == d && mv[0] == old[j + m] && mv[2] == (j == k0 ? rem : 0) && mv[3] == bs);
    }
    auto& r = rows[mv[1]];
    r.resize(bs);
    for (int i = mv[2]; i < mv[3]; ++i) ++r[i];
  }
  REQUIRE((int)rows.size() == nb - m - k0);
  for (const auto& r : rows)
    for (int c : r.second) REQUIRE(c == 1);
  check(s, blocks);  // with the released blocks still held
  if (rng() % 4) s.shift_done();
}

static void drive(std::mt19937& rng, bool cache, int steps) {
  const int blocks = 41, bs = 64, slots = 5, maxb = 10;
  Scheduler s(blocks, bs, slots, 600, maxb, 64, cache, 8);
  long long next = 1;
  std::map<long long, std::pair<std::vector<int>, int>> known;  // id -> prompt, max_new
  int shifts = 0;
  for (int step = 0; step < steps; ++step) {
    const int op = rng() % 9;
    if (op == 0 || op == 1) {
      const int n = 1 + rng() % 400, m = 1 + rng() % 300;
      const auto p = prompt(rng, n);
      if ((n + m + bs - 1) / bs > maxb) {
        REQUIRE(throws([&] { s.add(next, n, m, p); }));
      } else {
        s.add(next, n, m, p);
        known[next] = {p, m};
      }
      ++next;
    } else if (op == 2) {
      s.admit();
      s.take_copies();
      s.copies_done();
    } else if (op == 3 && s.num_running() > 0) {
      const auto run = s.running();
      s.publish(run[rng() % run.size()]);
    } else if (op == 4 && s.num_running() > 0) {
      const auto run = s.running();
      s.grow(run[rng() % run.size()], 1 + rng() % (bs * maxb + 100));
    } else if ((op == 5 || op == 8) && s.num_running() > 0) {
      const auto run = s.running();
      shift_one(s, rng, run[rng() % run.size()], blocks, bs);
      ++shifts;
    } else if (op == 6 && s.num_running() > 0 && rng() % 2) {
      s.shift_done();
      const long long id = s.youngest_first().front();
      auto& k = known.at(id);
      std::vector<int> p = k.first;
      for (int i = rng() % 40; i > 0; --i) p.push_back(rng() % 200);
      const int m = std::max(1, k.second - (int)(p.size() - k.first.size()));
      if (((int)p.size() + m + bs - 1) / bs <= maxb) {
        s.preempt(id, (int)p.size(), m, p);
        k = {p, m};
      }
    } else if (op == 7 && !known.empty()) {
      auto it = known.begin();
      std::advance(it, rng() % known.size());
      s.finish(it->first);
      known.erase(it);
    }
    check(s, blocks);
  }
  REQUIRE(shifts > steps / 20);
  for (const auto& k : known) s.finish(k.first);
  s.copies_done();
  s.shift_done();
  for (const auto& n : s.prefix_nodes()) REQUIRE(n[1] == 0);  // every reference is back
  s.reset_prefix_cache();
  REQUIRE(s.cached_blocks() == 0 && s.free_blocks() == blocks - 1 && s.num_running() == 0 && s.num_waiting() == 0);
}

int main() {
  std::mt19937 rng(97531);
  for (bool cache : {false, true, true}) drive(rng, cache, 4000);
  std::puts("context shift selftest ok");
  return 0;
}
