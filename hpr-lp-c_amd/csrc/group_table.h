// group_table.h -- the host side of a group recording (kernels.h: GroupLaunches; DESIGN.md "Many small LPs", group launches): which
// stages are issued in which order, where the tables of a run lie in its one block, and the resulting list of launches.  Host only:
// no HIP header, no device call (hprlp_group_table_selftest runs without a GPU, and tools/group_pack_check.cpp runs the same code
// under the host sanitizers).  kernels.hip keeps the typed tasks, copies the block and issues the list.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace hprlp {

// How the workgroups of a group kernel find their task.
enum GridRule : int {
    kGridMapped = 0,     // a {task, lb} map: the member's own grid per task, workgroup lb of it
    kGridReduce = 1,     // reduce_blocks workgroups per task (task = blockIdx.x / reduce_blocks), no map
    kGridPerTask = 2,    // one workgroup per task
    kGridPerThread = 3,  // one thread per task
};

constexpr size_t kTableAlign = 16;  // bytes: every table and map starts on such a boundary of the block

struct GroupLaunch {  // one launch of a run, in issue order
    int kind, stage;  // the kind's place in the recorder's list; the stage that holds its tasks
    int ntasks, nwg;
    size_t tasks, map;  // offsets in the block (map: kGridMapped only)
    bool own;           // no table: the caller issues the member's own launch
};

class GroupTable {
  public:
    // own_launches: a kind that holds ONE task in a stage takes no table where the caller says it has a launch of the member's own
    // (add's `own`); without it every kind present gets its table.
    GroupTable(bool own_launches, int reduce_blocks, int threads);
    bool own_launches() const { return own_; }

    // ---- the stages of a recording.  note() marks a kind present in the open stage; next_stage() closes the open stage unless
    // nothing was recorded in it; repeat_last(n, times) issues the last n closed stages `times` times in a row, tables once.
    int open_stage() const { return static_cast<int>(present_.size()) - 1; }
    void note(int kind);
    void next_stage();
    void repeat_last(int nseg, int times);  // throws std::invalid_argument for stages that were not recorded
    int recorded_launches() const;          // what finish() lists for the stages held now: one per kind present and stage issued

    // ---- one run: begin(), add() stage by stage each kind present in the fixed order of the kinds, finish()
    void begin();
    size_t put(const void *p, size_t n);                          // n bytes into the block, returns their offset
    size_t put_map(const int *grids, int ntasks, int *nwg);       // {task, lb} for lb < grids[task], task by task
    // The tasks of one kind in one stage (grids: kGridMapped, the member's own grid per task).  own: the caller can issue these
    // tasks as a member's own launch -- honoured under own_launches only.  Stages in ascending order.
    void add(int stage, int kind, GridRule rule, const void *tasks, size_t task_bytes, int ntasks, const int *grids, bool own);
    const std::vector<GroupLaunch> &finish();  // the launches in issue order; the recording starts over
    const std::vector<char> &bytes() const { return bytes_; }

  private:
    bool own_;
    int reduce_blocks_, threads_;
    std::vector<uint64_t> present_ = std::vector<uint64_t>(1);  // per stage, the open one last: bit `kind`
    std::vector<int> order_;                                    // closed stages as they are issued
    std::vector<char> bytes_;
    std::vector<GroupLaunch> made_;  // a run's launches stage by stage, each stage once; first_[i] .. first_[i + 1]: stage i's
    std::vector<size_t> first_;
    std::vector<GroupLaunch> list_;
};

// The normal iterations of a round as SEGMENTS (many.cpp: wide members; DESIGN.md "Many small LPs", wide members).  Members of one
// round owe different numbers of iterations (a restart costs one, max_iter cuts the last round, iterate_many takes any counts).
// With c_1 < ... < c_J the distinct positive counts and c_0 = 0, segment j runs c_j - c_{j-1} iterations with the members whose
// count is >= c_j: every member runs its own count, in a row, and the members of a segment share its launches.  len[j] and
// min_count[j] = c_j are appended in ascending order; a count <= 0 is in no segment.  Returns J.
int group_iteration_plan(const int *counts, int n, std::vector<int> &len, std::vector<int> &min_count);

}  // namespace hprlp

extern "C" int hprlp_group_table_selftest(void);  // 0, or the number of the check that failed
// group_iteration_plan through plain arrays of `cap` entries each.  Returns the number of segments, or -1: a null array, n < 0, a
// negative count, or more segments than cap.
extern "C" int hprlp_group_iteration_plan(const int *counts, int n, int *seg_len, int *seg_min_count, int cap);
