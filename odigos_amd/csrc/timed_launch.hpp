// timed_launch.hpp — one launch between a profile's start and stop events
// (HIP-free: Engine::timed instantiates it with the engine, tests/
// timed_check.cpp with a fake event pool).  Prof has
//   bool profiling
//   Mark prof_begin(name, st)   two events taken from the pool, the first recorded
//   void prof_end(Mark&, st)    the second recorded, the pair kept for the read-out
//   void prof_drop(Mark&)       both events handed back to the pool
//   int  launch_status()        the runtime's launch error as a return code
// launch() queues the work and returns nothing, or an int that ends the step
// when it is not 0.  A failing step hands its two events back before the code
// is returned, so the pool does not shrink by two per failure.
#pragma once
#include <type_traits>
#include <utility>

namespace ose {

template <class F>
int run_launch(F&& launch) {
  if constexpr (std::is_void_v<decltype(launch())>) {
    launch();
    return 0;
  } else {
    return launch();
  }
}

template <class Prof, class Stream, class F>
int timed_launch(Prof& p, const char* name, Stream st, F&& launch) {
  if (!p.profiling) {
    const int rc = run_launch(std::forward<F>(launch));
    return rc ? rc : p.launch_status();
  }
  auto mark = p.prof_begin(name, st);
  int rc = run_launch(std::forward<F>(launch));
  if (!rc) rc = p.launch_status();
  if (rc) p.prof_drop(mark);
  else p.prof_end(mark, st);
  return rc;
}

}  // namespace ose
