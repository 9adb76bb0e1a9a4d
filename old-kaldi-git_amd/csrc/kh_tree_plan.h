// kh_tree_plan.h - the host plan of kh_tree_acc_stats (csrc/kh_tree.hip): plain C++, no HIP, so that the check, the sort and the
// work list are tested on the CPU (tests/test_tree_plan_host.py).
//
//   Check    every frame's event id lies in -1 ... num_events - 1 (-1: the frame is not used); the message names the frame
//   Build    a stable counting sort of the used frames by event: within an event the frames stay in ascending frame order,
//            which is the order the reference adds them in; the run of event e is sorted_row[event_offsets[e] ...
//            event_offsets[e + 1]); then the work list, one item per (event with a frame, block of kCols columns), the events
//            by falling run length (ties by rising event id) so that the long runs - the silence events of a recipe, thousands
//            of frames each where a triphone event has a handful - are launched first and do not form the tail
#ifndef KH_TREE_PLAN_H_
#define KH_TREE_PLAN_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace kh_tree {

constexpr int kCols = 64;   // columns of a work item: a lane each

struct Plan {
  std::vector<int32_t> sorted_row;      // [used frames] frame indices, by event, ascending within an event
  std::vector<int32_t> event_offsets;   // [num_events + 1] into sorted_row
  std::vector<int32_t> work_event;      // [items] longest run first
  std::vector<int32_t> work_block;      // [items] the item's columns are kCols * work_block ... (+ kCols, or to D)
  int32_t used = 0;                     // frames with an event
  int32_t events_used = 0;              // events with a frame
  int32_t longest = 0;                  // frames of the longest run
};

inline int ColumnBlocks(int D) { return (D + kCols - 1) / kCols; }

// false with *err set when a frame names an event the call does not have
inline bool Check(int T, const int32_t *frame_event, int num_events, std::string *err) {
  for (int t = 0; t < T; t++)
    if (frame_event[t] < -1 || frame_event[t] >= num_events) {
      char buf[160];
      std::snprintf(buf, sizeof(buf), "frame %d names event %d, the call has %d events (-1: frame not used)", t, frame_event[t], num_events);
      *err = buf;
      return false;
    }
  return true;
}

// the frames (already checked) by event, and the work list
inline void Build(int T, const int32_t *frame_event, int num_events, int D, Plan *plan) {
  plan->event_offsets.assign(static_cast<size_t>(num_events) + 1, 0);
  for (int t = 0; t < T; t++)
    if (frame_event[t] >= 0) plan->event_offsets[frame_event[t] + 1]++;
  for (int e = 0; e < num_events; e++) plan->event_offsets[e + 1] += plan->event_offsets[e];
  plan->used = plan->event_offsets[num_events];
  plan->sorted_row.resize(plan->used);
  std::vector<int32_t> next(plan->event_offsets.begin(), plan->event_offsets.end() - 1);
  for (int t = 0; t < T; t++)
    if (frame_event[t] >= 0) plan->sorted_row[next[frame_event[t]]++] = t;
  std::vector<int32_t> order;
  for (int e = 0; e < num_events; e++)
    if (plan->event_offsets[e + 1] > plan->event_offsets[e]) order.push_back(e);
  const std::vector<int32_t> &off = plan->event_offsets;
  std::stable_sort(order.begin(), order.end(), [&off](int32_t a, int32_t b) { return off[a + 1] - off[a] > off[b + 1] - off[b]; });
  plan->events_used = static_cast<int32_t>(order.size());
  plan->longest = order.empty() ? 0 : off[order[0] + 1] - off[order[0]];
  const int blocks = ColumnBlocks(D);
  plan->work_event.clear();
  plan->work_block.clear();
  plan->work_event.reserve(order.size() * blocks);
  plan->work_block.reserve(order.size() * blocks);
  for (int32_t e : order)
    for (int b = 0; b < blocks; b++) {
      plan->work_event.push_back(e);
      plan->work_block.push_back(b);
    }
}

}  // namespace kh_tree
#endif  // KH_TREE_PLAN_H_
