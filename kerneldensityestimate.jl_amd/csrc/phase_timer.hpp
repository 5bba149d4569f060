// phase_timer.hpp -- kdehip_profile_phase_read: device time of the blocking entries either side of the product
// (LOOCV search, direct evaluation, GPU tree build), bracketed with HIP events on the stream their launches go to while
// kdehip_profile_sampler is on.  Diagnostics only (bench.py --frow); off: one relaxed load per phase.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kdehip {

// (3..5: the three passes of kdehip_evaluate_tol, each between two events of its own -- evaltol.hip; 6..8: those of
// kdehip_knn -- knn.hip; 9: the passes of a refit, copy to examination -- refit.hip)
enum ProfilePhase : int { kPhaseLoocv = 0, kPhaseEvaluate = 1, kPhaseTreeBuild = 2, kPhaseTolBox = 3, kPhaseTolPlan = 4,
                          kPhaseTolSweep = 5, kPhaseKnnBox = 6, kPhaseKnnPlan = 7, kPhaseKnnSweep = 8, kPhaseRefit = 9, kPhaseCount = 10 };
bool profile_phases_on();                        // devmem.cpp (set by kdehip_profile_sampler)
void profile_phases_set(bool on);
void profile_phase_add(int which, double ms);

class PhaseTimer {
 public:
  PhaseTimer(int which, hipStream_t st) : which_(which), st_(st) {
    if (!profile_phases_on()) return;
    if (hipEventCreate(&a_) != hipSuccess || hipEventCreate(&b_) != hipSuccess) { drop(); return; }
    if (hipEventRecord(a_, st_) != hipSuccess) drop();
  }
  PhaseTimer(const PhaseTimer &) = delete;
  PhaseTimer &operator=(const PhaseTimer &) = delete;
  void stop() { if (a_ && hipEventRecord(b_, st_) == hipSuccess) stopped_ = true; }
  // once the stream has been synchronised by the caller
  void collect() {
    float ms = 0.0f;
    if (a_ && stopped_ && hipEventElapsedTime(&ms, a_, b_) == hipSuccess) profile_phase_add(which_, ms);
    drop();
  }
  ~PhaseTimer() { drop(); }

 private:
  void drop() {
    if (a_) (void)hipEventDestroy(a_);
    if (b_) (void)hipEventDestroy(b_);
    a_ = b_ = nullptr;
  }
  int which_;
  hipStream_t st_;
  hipEvent_t a_ = nullptr, b_ = nullptr;
  bool stopped_ = false;
};

// four events around three consecutive passes of one call while kdehip_profile_sampler is on (phases first .. first + 2);
// otherwise none
class PassMarks {
 public:
  PassMarks(int first, bool wanted) : first_(first) {
    if (!wanted || !profile_phases_on()) return;
    for (hipEvent_t &e : ev_)
      if (hipEventCreate(&e) != hipSuccess) { e = nullptr; drop(); return; }
    on_ = true;
  }
  PassMarks(const PassMarks &) = delete;
  PassMarks &operator=(const PassMarks &) = delete;
  ~PassMarks() { drop(); }
  hipEvent_t *events() { return on_ ? ev_ : nullptr; }
  // once the stream has been synchronised by the caller
  void collect() {
    for (int k = 0; on_ && k < 3; ++k) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, ev_[k], ev_[k + 1]) == hipSuccess) profile_phase_add(first_ + k, ms);
    }
    drop();
  }

 private:
  void drop() {
    for (hipEvent_t &e : ev_) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    on_ = false;
  }
  int first_;
  hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
  bool on_ = false;
};

}  // namespace kdehip
