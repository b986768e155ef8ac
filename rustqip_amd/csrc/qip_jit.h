// qip_jit.h — the run-time compiler (qip_jit.hip) as the rest of the library calls it: a job goes in, a resident kernel is
// launched.  Its mutexes, caches and counters stay inside the unit (the locking rule is at the top of qip_jit.hip).
// Part of qip_internal.h, which includes it after the headers it needs.
#pragma once
struct qip_hip_state;

// One kernel to have: the source text of a segment and whether products may fuse into sums (option "tile_fma").
struct JitJob {
  std::string src;
  bool fma = false;
  bool operator==(const JitJob& o) const { return fma == o.fma && src == o.src; }
};

// global options, written by qip_hip_set_global_option / qip_hip_dist_create
extern int64_t g_jit_disk;   // "jit_disk_cache": code objects are kept on disk
extern int64_t g_jit_procs;  // "jit_procs": helper processes; 0 = automatic (the CPUs this process may use, at most 16), 1 = in process only
extern int64_t g_jit_world;  // ranks that share this host's CPUs: automatic jit_procs is divided by it
int jit_set_cache_cap(int64_t cap);   // "jit_cache_cap"
int jit_set_disk_cap_mb(int64_t mb);  // "jit_disk_cap_mb"

// The job's resident kernel, compiled on a miss, handed to `launch` while the cache is locked (no eviction can unload it between
// the lookup and the launch).  `launch` null: the kernel is only made resident — or, with `collect`, a miss is appended there
// and nothing is compiled (the pass that gathers a plan's new segments for jit_prepare / jit_lookup).
int jit_run(qip_hip_state* s, const JitJob& job, const std::function<int(hipFunction_t)>& launch, std::vector<JitJob>* collect = nullptr);
// Every job resident: from the disk cache, helper processes or this process.  (Both drop duplicates from `jobs`.)
int jit_prepare(qip_hip_state* s, std::vector<JitJob>& jobs);
// Nothing is compiled: all of `jobs` on disk -> all resident; otherwise nothing is loaded and the missing ones are in `misses`.
int jit_lookup(qip_hip_state* s, std::vector<JitJob>& jobs, std::vector<JitJob>* misses);
void jit_compile_in_background(const std::vector<JitJob>& misses);  // helper processes nobody waits for
int jit_obtain_code(const std::vector<JitJob>& jobs, std::vector<std::vector<char>>* code);  // device-free: the code objects

// What is known of a plan by its fingerprint: all its segments were made resident and nothing has been evicted since; a lookup
// found it incomplete less than 1.5 s ago; nothing.
enum class JitPlanMemo { kUnknown, kWarm, kColdRecently };
JitPlanMemo jit_plan_query(uint64_t fingerprint);
void jit_plan_mark_warm(uint64_t fingerprint);
void jit_plan_mark_cold(uint64_t fingerprint);

// A hipGraph that names resident kernels holds the generation it was recorded under (it moves with every eviction) and is
// launched through jit_launch_if_current: `*stale` = the cache has evicted since, nothing was launched, record again.
void jit_capture_scope(int delta);  // +1 / -1 around a stream capture: nothing is evicted while any thread records
uint64_t jit_cache_generation();
int jit_launch_if_current(uint64_t generation, const std::function<int()>& launch, bool* stale);
