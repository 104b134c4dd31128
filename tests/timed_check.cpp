// Host check of timed_launch.hpp (what Engine::timed runs) against a fake
// event pool: a launch that fails, by its own code or by the runtime's launch
// status, leaves the pool the size it was; a launch that succeeds keeps its
// two events for the read-out; with profiling off no event is touched and the
// launch and its status check still run.  Run by test_slab.py.
#include <cstdio>
#include <string>
#include <vector>

#include "../odigos_amd/csrc/timed_launch.hpp"

namespace {
struct FakeProf {
  struct Mark { const char* name; int a, b; };
  bool profiling = false;
  std::vector<int> pool;      // free events
  std::vector<Mark> kept;     // finished pairs, waiting for the read-out
  std::string log;            // what was recorded on the "stream", in order
  int next_event = 100, status = 0, status_calls = 0;
  int take() {
    if (pool.empty()) return next_event++;
    const int ev = pool.back();
    pool.pop_back();
    return ev;
  }
  Mark prof_begin(const char* name, int) {
    Mark m{name, take(), take()};
    log += "a";
    return m;
  }
  void prof_end(Mark& m, int) {
    log += "b";
    kept.push_back(m);
  }
  void prof_drop(Mark& m) {
    pool.push_back(m.a);
    pool.push_back(m.b);
  }
  int launch_status() {
    status_calls++;
    return status;
  }
  // the events this profile owns: free, or kept for the read-out
  size_t owned() const { return pool.size() + 2 * kept.size(); }
};

int bad(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}
}  // namespace

int main() {
  using ose::timed_launch;
  // profiling off: the launch runs, its status is checked, no event is taken
  {
    FakeProf p;
    p.pool = {1, 2, 3, 4};
    int ran = 0;
    if (timed_launch(p, "k", 0, [&] { ran++; }) != 0 || ran != 1 || p.status_calls != 1) return bad("off: a void launch");
    p.status = 9;
    if (timed_launch(p, "k", 0, [&] { ran++; }) != 9 || ran != 2) return bad("off: the launch status is returned");
    if (timed_launch(p, "k", 0, [&] { ran++; return 5; }) != 5 || p.status_calls != 2)
      return bad("off: the launch's own code comes first, with no status check behind it");
    if (p.pool.size() != 4 || !p.kept.empty() || !p.log.empty()) return bad("off: an event was touched");
  }
  // profiling on, a warm pool: a success keeps two events between begin and end
  FakeProf p;
  p.profiling = true;
  p.pool = {1, 2, 3, 4};
  if (timed_launch(p, "ok", 0, [&] { p.log += "L"; }) != 0) return bad("on: a success");
  if (p.log != "aLb" || p.kept.size() != 1 || p.pool.size() != 2 || std::string(p.kept[0].name) != "ok")
    return bad("on: begin, launch, end, and the pair kept under its name");
  // failing launches, many times over: the pool never shrinks, nothing is kept, no stop event recorded
  const size_t owned = p.owned(), free_before = p.pool.size();
  for (int k = 0; k < 100; k++) {
    p.status = 7;
    if (timed_launch(p, "bad", 0, [&] { p.log += "L"; }) != 7) return bad("on: the launch status is returned");
    p.status = 0;
    if (timed_launch(p, "bad", 0, [&]() -> int { return 3; }) != 3) return bad("on: the launch's own code is returned");
    if (p.pool.size() != free_before || p.owned() != owned || p.kept.size() != 1)
      return bad("on: a failing launch changed the pool's size");
  }
  if (p.next_event != 100) return bad("on: a failing launch made the pool create events");
  if (p.log.find('b', 3) != std::string::npos) return bad("on: a failing launch recorded its stop event");
  // an empty pool: the two events a failure created go to the pool, and the next launch reuses them
  FakeProf q;
  q.profiling = true;
  q.status = 7;
  if (timed_launch(q, "bad", 0, [] {}) != 7 || q.pool.size() != 2 || q.next_event != 102) return bad("cold: a failure");
  q.status = 0;
  if (timed_launch(q, "ok", 0, [] {}) != 0 || q.next_event != 102 || !q.pool.empty() || q.kept.size() != 1)
    return bad("cold: the next launch reuses the failure's events");
  std::puts("OK");
  return 0;
}
