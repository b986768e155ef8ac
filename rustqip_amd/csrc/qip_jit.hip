// qip_jit.hip — the run-time compiler: hiprtc, the code objects on disk, the helper processes, the resident kernels, the plan memo.
// It knows nothing about circuits: a job is a source text and a contraction flag (JitJob, qip_jit.h).
//
// LOCKING.  The state below is process-global while handles are per thread — "separate handles are independent"
// (include/qip_hip.h) has to hold for two threads that both run compiled segments.  Two mutexes:
//   g_jit_mutex  guards the resident kernel cache, the directory setting, every counter and the plan memo.  A function
//                named *_locked is called with it held.  A kernel is launched with it held too (jit_run,
//                jit_launch_if_current): an eviction synchronises the device and unloads the module, so a function handle
//                that was looked up and then launched outside the lock could dangle.
//   g_rtc_mutex  guards g_rtc and every hiprtc call (they are not documented to be re-entrant); taken only inside
//                hiprtc_handle / hiprtc_compile.  It costs nothing: comgr serialises one process's compilations anyway (r5 note below).
// Order: g_jit_mutex, then g_rtc_mutex, never the reverse — nothing that holds g_rtc_mutex calls back into the cache.
// Disk reads and writes, hashing and the helper processes need neither: files appear by rename, names are unique per
// process and serial, and what a pass counted is added to the counters in one locked step (JitTally).
#include "qip_internal.h"

#include <atomic>
#include <mutex>
#include <set>
#include <thread>

#include <cerrno>
#include <climits>
#include <dirent.h>
#include <fcntl.h>
#include <sched.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>
extern char** environ;

static const char kKernelsHeaderSrc[] =
#include "qip_kernels_embed.inc"
    ;

struct Hiprtc {
  void* handle = nullptr;
  int (*CreateProgram)(void**, const char*, const char*, int, const char**, const char**) = nullptr;
  int (*CompileProgram)(void*, int, const char**) = nullptr;
  int (*GetProgramLogSize)(void*, size_t*) = nullptr;
  int (*GetProgramLog)(void*, char*) = nullptr;
  int (*GetCodeSize)(void*, size_t*) = nullptr;
  int (*GetCode)(void*, char*) = nullptr;
  int (*DestroyProgram)(void**) = nullptr;
};
static Hiprtc g_rtc;
static std::mutex g_jit_mutex, g_rtc_mutex;  // (see LOCKING above)
// under g_rtc_mutex
static int hiprtc_load_locked() {
  if (g_rtc.handle) return QIP_OK;
  void* h = nullptr;
  for (const char* name : {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"}) {
    h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (h) break;
  }
  if (!h) return fail(QIP_ERR_UNSUPPORTED, "option tile_jit needs libhiprtc: %s", dlerror());
#define RSYM(field, name)                                                           \
  do {                                                                              \
    *(void**)(&g_rtc.field) = dlsym(h, name);                                       \
    if (!g_rtc.field) return fail(QIP_ERR_UNSUPPORTED, "libhiprtc lacks %s", name); \
  } while (0)
  RSYM(CreateProgram, "hiprtcCreateProgram");
  RSYM(CompileProgram, "hiprtcCompileProgram");
  RSYM(GetProgramLogSize, "hiprtcGetProgramLogSize");
  RSYM(GetProgramLog, "hiprtcGetProgramLog");
  RSYM(GetCodeSize, "hiprtcGetCodeSize");
  RSYM(GetCode, "hiprtcGetCode");
  RSYM(DestroyProgram, "hiprtcDestroyProgram");
#undef RSYM
  g_rtc.handle = h;
  return QIP_OK;
}
// the loaded libhiprtc, or null (the message is in g_last_error)
static void* hiprtc_handle() {
  std::lock_guard<std::mutex> lock(g_rtc_mutex);
  return hiprtc_load_locked() == QIP_OK ? g_rtc.handle : nullptr;
}
// source -> code object (host only: works without a device, which is how the CPU tests cover it)
static int hiprtc_compile(const std::string& src, bool fma, std::vector<char>* code) {
  std::lock_guard<std::mutex> lock(g_rtc_mutex);
  QCHK(hiprtc_load_locked());
  void* prog = nullptr;
  const char* hdr_src[1] = {kKernelsHeaderSrc};
  const char* hdr_name[1] = {"qip_kernels.h"};
  if (g_rtc.CreateProgram(&prog, src.c_str(), "qip_segment.hip", 1, hdr_src, hdr_name) != 0)
    return fail(QIP_ERR_DEVICE, "hiprtcCreateProgram failed");
  // as rustqip_amd/build.py; `fma` (option "tile_fma", only honoured for tile = 2, whose bar is 1e-12 anyway): products may
  // fuse into the sums that consume them (v_fma_f64): a complex product is 4 instead of 6 vector instructions
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", fma ? "-ffp-contract=fast" : "-ffp-contract=off", "-fno-slp-vectorize"};
  const int rc = g_rtc.CompileProgram(prog, (int)(sizeof opts / sizeof opts[0]), opts);
  if (rc != 0) {
    size_t n = 0;
    g_rtc.GetProgramLogSize(prog, &n);
    std::string log(n + 1, '\0');
    if (n) g_rtc.GetProgramLog(prog, &log[0]);
    g_rtc.DestroyProgram(&prog);
    return fail(QIP_ERR_DEVICE, "hiprtc could not compile a tile segment (%d): %.800s", rc, log.c_str());
  }
  size_t sz = 0;
  g_rtc.GetCodeSize(prog, &sz);
  code->resize(sz);
  g_rtc.GetCode(prog, code->data());
  g_rtc.DestroyProgram(&prog);
  return QIP_OK;
}

// ---------------------------------------------------------------------------------------
// r5: code objects on disk, and a plan's new segments compiled in helper PROCESSES.
//  * hiprtc costs ~0.45 s per 11-bit segment and ~1.3 s per wide one, and the code-object manager behind it serialises the
//    compilations of one process (r4, 8 host cores: 18 narrow segments took 8.4 s on 8 threads against 9.0 s on one, 12 wide ones
//    14.3 s against 15.3 s).  Separate processes do scale (measured on 8 cores: four
//    processes compile four plans in the time of one), so the segments of a plan that are new are written out as source files,
//    `qip_jitc` (a 30-line host program next to the library; it calls qip_hip_jit_compile_file below) is spawned up to
//    "jit_procs" times, and the code objects come back through the disk cache.  No helper, one new segment, or jit_procs = 1:
//    the compilation happens in this process as before.
//  * every code object is kept under $QIP_HIP_CACHE_DIR (default $XDG_CACHE_HOME/qip_hip or ~/.cache/qip_hip; "off" or an
//    empty value disables), named by a 128-bit hash of compiler version + flags + the embedded kernel header + the source text,
//    written to a temporary name and renamed (readers never see half a file; two processes that compile the same segment just
//    both succeed).  A second process loads instead of compiling: ~1 ms per segment.
//  * r6, what is TRUSTED: a code object found on disk ends up on the GPU, so the cache only ever reads what this user wrote.
//    The directory must be owned by the effective uid and writable by nobody else (an existing directory that is not: no disk
//    cache — the default rule falls back to "none", qip_hip_jit_set_cache_dir reports the reason); a file must be a regular
//    file (no symlink), owned by the uid, not group/world-writable; its header carries the source length, the second word of
//    the key and a hash of the CODE BYTES, all checked on load.  Anything odd is a miss (and a recompilation that overwrites
//    the file), never an error, never a load.  The key names the compiler by the ROCm installation the helper processes use
//    ($ROCM_PATH or /opt/rocm: its release and the sizes of its libhiprtc / libamd_comgr — see jit_compiler_identity; a host
//    program that has another ROCm's libraries loaded, PyTorch for one, hands even single segments to a helper).
//  * r6, bounded: after a store the directory is trimmed to "jit_disk_cap_mb" (global option; $QIP_HIP_CACHE_MAX_MB; default
//    1024) — oldest modification time first (a hit refreshes it), stale temporaries with them.
// ---------------------------------------------------------------------------------------
int64_t g_jit_disk = 1, g_jit_procs = 0, g_jit_world = 1;  // the global options (qip_jit.h)
static std::string g_jit_dir;           // resolved cache directory ("" = none)
static bool g_jit_dir_resolved = false;
static uint64_t g_jit_disk_hits = 0, g_jit_disk_stores = 0, g_jit_helper_procs = 0, g_jit_helper_segments = 0;
static double g_jit_load_ms = 0;
static uint64_t g_jit_background_segments = 0;  // segments handed to background helpers (option tile_auto, one-shot callers)

struct JitHash {
  uint64_t a = 0, b = 0;
};
static uint64_t hash_fnv(const char* p, size_t n, uint64_t h) {
  for (size_t i = 0; i < n; ++i) {
    h ^= (unsigned char)p[i];
    h *= 1099511628211ull;
  }
  return h;
}
static uint64_t hash_mix(const char* p, size_t n, uint64_t h) {  // an independent second word: 8 bytes at a time
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, p + i, 8);
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
  }
  for (; i < n; ++i) {
    h = (h ^ (unsigned char)p[i]) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 31;
  }
  return h;
}
static const char* jit_flags_text(bool fma) {
  return fma ? "gfx950 -O3 c++17 contract=fast no-slp" : "gfx950 -O3 c++17 contract=off no-slp";
}
// The compiler a key names.  New segments are compiled by helper processes (qip_jitc): fresh processes that load the system's
// ROCm — whatever THIS process has loaded.  A host program that imported PyTorch first carries PyTorch's own bundled libhiprtc /
// libamd_comgr / HIP runtime (another ROCm release), so "as loaded here" named a different compiler than the one that wrote the
// files: the helpers' objects failed the header check and every segment was compiled a second time in process (r6: bench.py's
// 207 segments, 93 s instead of 31), and a process without PyTorch never found what a process with PyTorch had cached.
// So the identity is that of the INSTALLATION the helpers use, read from its files: $ROCM_PATH or /opt/rocm — the release
// (.info/version) and the byte sizes of libhiprtc / libamd_comgr there (an updated ROCm changes at least one of the three).
// Only when no such installation is found does the key fall back to what this process has loaded (hiprtc's version, the HIP
// runtime's version, the sizes of the two shared objects as loaded).
static std::string g_jit_canonical_hiprtc;  // real path of the installation's libhiprtc ("" = fell back to as-loaded)
static std::string jit_compiler_identity() {
  for (const char* root : {(const char*)getenv("ROCM_PATH"), "/opt/rocm"}) {
    if (!root || !*root) continue;
    const std::string r = root;
    struct stat st_rtc, st_comgr;
    if (stat((r + "/lib/libhiprtc.so").c_str(), &st_rtc) != 0 || stat((r + "/lib/libamd_comgr.so").c_str(), &st_comgr) != 0) continue;
    char release[64] = "?";
    if (FILE* f = fopen((r + "/.info/version").c_str(), "r")) {
      if (fscanf(f, "%63s", release) != 1) strcpy(release, "?");
      fclose(f);
    }
    char real[PATH_MAX];
    if (realpath((r + "/lib/libhiprtc.so").c_str(), real)) g_jit_canonical_hiprtc = real;
    char v[224];
    snprintf(v, sizeof v, "qipjit3 rocm %s libhiprtc %lld comgr %lld ", release, (long long)st_rtc.st_size, (long long)st_comgr.st_size);
    return v;
  }
  int major = 0, minor = 0, rt = 0;
  long long sz_rtc = 0, sz_comgr = 0;
  if (void* rtc = hiprtc_handle()) {  // (part of every key: always asked, so that keys do not depend on who hashes first)
    int (*ver)(int*, int*) = nullptr;
    *(void**)(&ver) = dlsym(rtc, "hiprtcVersion");
    if (ver) (void)ver(&major, &minor);
    Dl_info info;
    struct stat st;
    if (ver && dladdr((void*)ver, &info) && info.dli_fname && stat(info.dli_fname, &st) == 0) sz_rtc = (long long)st.st_size;
    // (loaded here if hiprtc has not done so yet — it does lazily, at its first compilation: the key must not depend on that)
    for (const char* name : {"libamd_comgr.so", "libamd_comgr.so.3", "/opt/rocm/lib/libamd_comgr.so"}) {
      void* comgr = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (!comgr) continue;
      void* sym = dlsym(comgr, "amd_comgr_get_version");
      if (sym && dladdr(sym, &info) && info.dli_fname && stat(info.dli_fname, &st) == 0) sz_comgr = (long long)st.st_size;
      break;  // (stays loaded: hiprtc needs it anyway)
    }
  }
  (void)hipRuntimeGetVersion(&rt);
  char v[160];
  snprintf(v, sizeof v, "qipjit2 hiprtc %d.%d runtime %d libhiprtc %lld comgr %lld ", major, minor, rt, sz_rtc, sz_comgr);
  return v;
}
// true when a compilation in THIS process would use another libhiprtc than the one the keys name (a host program that brought its
// own ROCm libraries): such a process sends even a single new segment to a helper, so that a file is what its name says
static bool jit_foreign_hiprtc_loaded() {
  static const bool foreign = [] {
    void* rtc = g_jit_canonical_hiprtc.empty() ? nullptr : hiprtc_handle();
    if (!rtc) return false;
    int (*ver)(int*, int*) = nullptr;
    *(void**)(&ver) = dlsym(rtc, "hiprtcVersion");
    Dl_info info;
    char real[PATH_MAX];
    if (!ver || !dladdr((void*)ver, &info) || !info.dli_fname || !realpath(info.dli_fname, real)) return false;
    return g_jit_canonical_hiprtc != real;
  }();
  return foreign;
}
static JitHash jit_hash(const std::string& src, bool fma) {
  static JitHash base = [] {  // the embedded header and the compiler's identity: once per process
    JitHash h;
    const std::string v = jit_compiler_identity();
    h.a = hash_fnv(v.data(), v.size(), 1469598103934665603ull);
    h.b = hash_mix(v.data(), v.size(), 0x243F6A8885A308D3ull);
    h.a = hash_fnv(kKernelsHeaderSrc, sizeof kKernelsHeaderSrc, h.a);
    h.b = hash_mix(kKernelsHeaderSrc, sizeof kKernelsHeaderSrc, h.b);
    return h;
  }();
  JitHash h = base;
  const char* f = jit_flags_text(fma);
  h.a = hash_fnv(f, strlen(f), h.a);
  h.b = hash_mix(f, strlen(f), h.b);
  h.a = hash_fnv(src.data(), src.size(), h.a);
  h.b = hash_mix(src.data(), src.size(), h.b);
  return h;
}
static bool mkdir_p(const std::string& dir) {
  struct stat st;
  if (stat(dir.c_str(), &st) == 0) return S_ISDIR(st.st_mode);
  const size_t slash = dir.find_last_of('/');
  if (slash != std::string::npos && slash > 0 && !mkdir_p(dir.substr(0, slash))) return false;
  return mkdir(dir.c_str(), 0700) == 0 || (stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode));
}
// A cache directory is used only when it belongs to this user and nobody else can write to it: what it holds is loaded onto the GPU.
static bool jit_dir_trusted(const std::string& dir, std::string* why) {
  struct stat st;
  if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) {
    if (why) *why = "not a directory";
    return false;
  }
  if (st.st_uid != geteuid()) {
    if (why) *why = "not owned by this user";
    return false;
  }
  if (st.st_mode & (S_IWGRP | S_IWOTH)) {
    if (why) *why = "writable by group or others";
    return false;
  }
  return access(dir.c_str(), W_OK | X_OK) == 0 || ((why ? (void)(*why = "not writable") : (void)0), false);
}
// under g_jit_mutex (or before any thread exists): where code objects are kept; "" = nowhere
static const std::string& jit_dir_locked() {
  if (g_jit_dir_resolved) return g_jit_dir;
  g_jit_dir_resolved = true;
  g_jit_dir.clear();
  std::string dir;
  if (const char* e = getenv("QIP_HIP_CACHE_DIR")) {
    if (!*e || !strcmp(e, "off") || !strcmp(e, "0")) return g_jit_dir;
    dir = e;
  } else if (const char* x = getenv("XDG_CACHE_HOME")) {
    if (*x) dir = std::string(x) + "/qip_hip";
  }
  if (dir.empty()) {
    const char* home = getenv("HOME");
    if (!home || !*home) return g_jit_dir;
    dir = std::string(home) + "/.cache/qip_hip";
  }
  if (mkdir_p(dir) && jit_dir_trusted(dir, nullptr)) g_jit_dir = dir;
  return g_jit_dir;
}
static std::string jit_disk_path(const std::string& dir, const JitHash& h) {
  char name[48];
  snprintf(name, sizeof name, "/%016llx%016llx.co", (unsigned long long)h.a, (unsigned long long)h.b);
  return dir + name;
}
struct JitFileHeader {
  char magic[8];
  uint64_t src_len, hash_b, code_len, code_hash;
};
static uint64_t jit_code_hash(const char* p, size_t n) { return hash_mix(p, n, 0x13198A2E03707344ull ^ (uint64_t)n); }
static bool jit_disk_read(const std::string& path, size_t src_len, const JitHash& h, std::vector<char>* code) {
  const int fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
  if (fd < 0) return false;
  struct stat st;
  bool ok = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_uid == geteuid() && !(st.st_mode & (S_IWGRP | S_IWOTH));
  JitFileHeader hd;
  auto read_all = [&](void* dst, size_t n) {
    char* q = (char*)dst;
    while (n) {
      const ssize_t got = read(fd, q, n);
      if (got < 0 && errno == EINTR) continue;
      if (got <= 0) return false;
      q += got;
      n -= (size_t)got;
    }
    return true;
  };
  ok = ok && read_all(&hd, sizeof hd) && !memcmp(hd.magic, "QIPJIT2", 8) && hd.src_len == src_len && hd.hash_b == h.b && hd.code_len > 0 &&
       hd.code_len < (1ull << 31) && (uint64_t)st.st_size == sizeof hd + hd.code_len;
  if (ok) {
    code->resize(hd.code_len);
    ok = read_all(code->data(), hd.code_len) && jit_code_hash(code->data(), code->size()) == hd.code_hash;
  }
  if (ok) (void)futimens(fd, nullptr);  // a hit refreshes the modification time: the trim below drops the oldest first
  close(fd);
  if (!ok) code->clear();
  return ok;
}
static std::atomic<unsigned> g_jit_tmp_serial{0};  // temporaries of one process never share a name (two handles may compile side by side)
static int64_t g_jit_disk_cap_mb = -1;             // global option "jit_disk_cap_mb"; -1 = $QIP_HIP_CACHE_MAX_MB or 1024
static uint64_t g_jit_disk_trimmed = 0;
static bool jit_disk_write(const std::string& path, size_t src_len, const JitHash& h, const std::vector<char>& code) {
  char suffix[64];
  snprintf(suffix, sizeof suffix, ".tmp.%ld.%u", (long)getpid(), g_jit_tmp_serial.fetch_add(1));
  const std::string tmp = path + suffix;
  const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
  if (fd < 0) return false;
  JitFileHeader hd;
  memcpy(hd.magic, "QIPJIT2", 8);
  hd.src_len = src_len;
  hd.hash_b = h.b;
  hd.code_len = code.size();
  hd.code_hash = jit_code_hash(code.data(), code.size());
  auto write_all = [&](const void* src, size_t n) {
    const char* q = (const char*)src;
    while (n) {
      const ssize_t put = write(fd, q, n);
      if (put < 0 && errno == EINTR) continue;
      if (put <= 0) return false;
      q += put;
      n -= (size_t)put;
    }
    return true;
  };
  bool ok = write_all(&hd, sizeof hd) && write_all(code.data(), code.size());
  ok = close(fd) == 0 && ok;
  if (ok) ok = rename(tmp.c_str(), path.c_str()) == 0;
  if (!ok) (void)unlink(tmp.c_str());
  return ok;
}
// Keep the directory under its bound: code objects by modification time, oldest first, until 90 % of the bound is left; and the
// temporaries (sources handed to helpers, half-written objects) that a killed process left behind more than an hour ago.
static void jit_disk_trim(const std::string& dir) {
  int64_t cap_mb = g_jit_disk_cap_mb;
  if (cap_mb < 0) {
    const char* e = getenv("QIP_HIP_CACHE_MAX_MB");
    cap_mb = e && *e ? atoll(e) : 1024;
  }
  if (cap_mb <= 0 || dir.empty()) return;
  DIR* d = opendir(dir.c_str());
  if (!d) return;
  struct Ent {
    std::string name;
    int64_t mtime_ns;
    uint64_t size;
  };
  std::vector<Ent> objs;
  uint64_t total = 0;
  const time_t now = time(nullptr);
  while (struct dirent* de = readdir(d)) {
    const std::string name = de->d_name;
    struct stat st;
    if (name == "." || name == ".." || lstat((dir + "/" + name).c_str(), &st) != 0 || !S_ISREG(st.st_mode)) continue;
    const bool obj = name.size() > 3 && name.compare(name.size() - 3, 3, ".co") == 0;
    if (obj) {
      objs.push_back({name, (int64_t)st.st_mtim.tv_sec * 1000000000ll + st.st_mtim.tv_nsec, (uint64_t)st.st_size});
      total += (uint64_t)st.st_size;
    } else if ((name.find(".co.tmp.") != std::string::npos || name.compare(0, 4, "seg.") == 0) && now - st.st_mtime > 3600) {
      (void)unlink((dir + "/" + name).c_str());
    }
  }
  closedir(d);
  const uint64_t cap = (uint64_t)cap_mb << 20;
  if (total <= cap) return;
  std::sort(objs.begin(), objs.end(), [](const Ent& a, const Ent& b) { return a.mtime_ns < b.mtime_ns; });
  for (const Ent& e : objs) {
    if (total <= cap / 10 * 9) break;
    if (unlink((dir + "/" + e.name).c_str()) == 0) {
      total -= e.size;
      g_jit_disk_trimmed += 1;
    }
  }
}
int jit_set_disk_cap_mb(int64_t mb) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  g_jit_disk_cap_mb = mb;
  return QIP_OK;
}

// Host only (no device): compile the segment source in `src_path` and leave the code object at `out_path` in the disk
// cache's file format.  This is what the helper processes run (tools/qip_jitc.c).
extern "C" int qip_hip_jit_compile_file(const char* src_path, int fma, const char* out_path) try {
  if (!src_path || !out_path) return fail(QIP_ERR_INVALID, "null path");
  FILE* f = fopen(src_path, "rb");
  if (!f) return fail(QIP_ERR_INVALID, "cannot read %s", src_path);
  std::string src;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) src.append(buf, got);
  fclose(f);
  std::vector<char> code;
  QCHK(hiprtc_compile(src, fma != 0, &code));
  // The requester named the file by ITS key (<32 hex digits>.co): the header repeats the key's second word so that the requester's
  // own check passes — the name is the contract, whatever this process would have computed.  Any other name: this process's key.
  JitHash h = jit_hash(src, fma != 0);
  {
    const char* base = strrchr(out_path, '/');
    base = base ? base + 1 : out_path;
    unsigned long long a = 0, b = 0;
    int used = 0;
    if (strlen(base) == 35 && sscanf(base, "%16llx%16llx%n", &a, &b, &used) == 2 && used == 32 && !strcmp(base + 32, ".co")) {
      h.a = a;
      h.b = b;
    }
  }
  if (!jit_disk_write(out_path, src.size(), h, code)) return fail(QIP_ERR_DEVICE, "cannot write %s", out_path);
  return QIP_OK;
} QIP_CATCH_ALL

// the CPUs this process may actually use: affinity mask, capped by the cgroup's CPU quota (the GPU boxes show 256 CPUs and grant 16)
static int usable_cpus() {
  int n = (int)std::max(1u, std::thread::hardware_concurrency());
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::max(1, CPU_COUNT(&set));
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    long long period = 0;
    if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
      const long long quota = atoll(q);
      if (quota > 0) n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
    }
    fclose(f);
  }
  return n;
}
static int jit_procs_effective() {
  if (g_jit_procs >= 1) return (int)std::min<int64_t>(g_jit_procs, 64);
  static const int cpus = usable_cpus();
  return std::max(1, std::min(16, cpus) / (int)std::max<int64_t>(1, g_jit_world));
}
// the helper program: $QIP_HIP_JITC, or `qip_jitc` next to this library
static std::string jit_helper_path() {
  if (const char* e = getenv("QIP_HIP_JITC")) return access(e, X_OK) == 0 ? std::string(e) : std::string();
  Dl_info info;
  if (!dladdr((void*)&qip_hip_jit_compile_file, &info) || !info.dli_fname) return std::string();
  std::string pth = info.dli_fname;
  const size_t slash = pth.find_last_of('/');
  pth = (slash == std::string::npos ? std::string(".") : pth.substr(0, slash)) + "/qip_jitc";
  return access(pth.c_str(), X_OK) == 0 ? pth : std::string();
}
// Write the sources of jobs[todo[*]] into `dir` and spawn up to `procs` helper processes over them, round robin; results land at
// out_paths[*] (the disk cache).  Returns the number of processes started.  Foreground: waits for them and removes the sources.
// `background`: returns at once — the helpers remove their own sources (qip_jitc -u) and a detached thread reaps them (it touches
// nothing of this library).  Failures are not reported from here: a foreground caller compiles whatever is still missing in this
// process, which also produces the message.  The sources go into the trusted directory and are created as strictly as everything
// else there: a new file of this user's, never through a link.
static size_t jit_spawn_helpers(const std::string& helper, const std::string& dir, size_t procs, const std::vector<JitJob>& jobs,
                                const std::vector<size_t>& todo, const std::vector<std::string>& out_paths, bool background) {
  std::vector<std::string> src_paths(jobs.size());
  std::vector<size_t> written;
  for (size_t i : todo) {
    char name[64];
    snprintf(name, sizeof name, "/seg.%ld.%u.%zu.hip", (long)getpid(), g_jit_tmp_serial.fetch_add(1), i);
    src_paths[i] = dir + name;
    const int fd = open(src_paths[i].c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW | O_CLOEXEC, 0600);
    if (fd < 0) continue;
    const bool ok = write(fd, jobs[i].src.data(), jobs[i].src.size()) == (ssize_t)jobs[i].src.size();
    if (close(fd) == 0 && ok) written.push_back(i);
    else (void)unlink(src_paths[i].c_str());
  }
  const size_t np = std::min(procs, written.size());
  std::vector<pid_t> pids;
  for (size_t k = 0; k < np; ++k) {
    std::vector<std::string> args = {helper};
    if (background) args.push_back("-u");
    for (size_t j = k; j < written.size(); j += np) {  // round robin: heavy and light segments alternate along a plan
      const size_t i = written[j];
      args.push_back(jobs[i].fma ? "1" : "0");
      args.push_back(src_paths[i]);
      args.push_back(out_paths[i]);
    }
    std::vector<char*> argv;
    for (std::string& a : args) argv.push_back(&a[0]);
    argv.push_back(nullptr);
    pid_t pid = 0;
    if (posix_spawn(&pid, helper.c_str(), nullptr, nullptr, argv.data(), environ) == 0) pids.push_back(pid);
  }
  auto reap = [pids]() {
    for (pid_t pid : pids) {
      int status = 0;
      while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {
      }
    }
  };
  if (background && !pids.empty()) {
    std::thread(reap).detach();
  } else {
    reap();
    for (size_t i : written) (void)unlink(src_paths[i].c_str());
  }
  return pids.size();
}

struct JitKernel {
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  uint64_t last_use = 0;
  int device = 0;
};
// key: device ordinal + compile flavour + source text.  Bounded: beyond g_jit_cache_cap entries (global option
// "jit_cache_cap", default 512 — a parameter sweep that changes matrix constants makes new sources without end) the least
// recently used kernels are unloaded, oldest first.  A kernel that is evicted while a captured hipGraph still names it would
// dangle, so programs hold the cache generation they were recorded under and re-record when it moved (qip_hip_program_run).
static std::map<std::string, JitKernel> g_jit_cache;
static uint64_t g_jit_clock = 0, g_jit_generation = 0;
static int64_t g_jit_cache_cap = 512;
static uint64_t g_jit_compiles = 0, g_jit_evictions = 0, g_jit_loaded = 0;  // (compiles: hiprtc runs of THIS process; loaded: kernels made resident)
static double g_jit_compile_ms = 0;
// Stream captures in progress in this process, on any handle (under g_jit_mutex).  Evicting synchronises the device and
// unloads modules: neither may happen while ANY thread records a graph, not only the evicting handle's own capture.
static int g_jit_captures_in_progress = 0;
void jit_capture_scope(int delta) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  g_jit_captures_in_progress += delta;
}

extern "C" int qip_hip_jit_stats2(qip_hip_jit_counters* out) try {
  if (!out) return fail(QIP_ERR_INVALID, "null output");
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  out->kernels_resident_total = g_jit_loaded;
  out->compiled = g_jit_compiles;
  out->compiled_by_helpers = g_jit_helper_segments;
  out->helper_processes = g_jit_helper_procs;
  out->disk_hits = g_jit_disk_hits;
  out->disk_stores = g_jit_disk_stores;
  out->compile_ms = g_jit_compile_ms;
  out->disk_load_ms = g_jit_load_ms;
  out->procs = jit_procs_effective();
  out->disk_cache = (g_jit_disk && !jit_dir_locked().empty()) ? 1 : 0;
  out->background_segments = g_jit_background_segments;
  out->disk_trimmed = g_jit_disk_trimmed;
  return QIP_OK;
} QIP_CATCH_ALL

// Where code objects are kept.  dir = NULL: back to the default ($QIP_HIP_CACHE_DIR, $XDG_CACHE_HOME/qip_hip, ~/.cache/qip_hip);
// "" : nowhere.  A directory that cannot be created or written is an error and leaves the setting unchanged.
extern "C" int qip_hip_jit_set_cache_dir(const char* dir) try {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  if (!dir) {
    g_jit_dir_resolved = false;
    (void)jit_dir_locked();
    return QIP_OK;
  }
  if (!*dir) {
    g_jit_dir.clear();
    g_jit_dir_resolved = true;
    return QIP_OK;
  }
  const std::string d = dir;
  std::string why = "cannot be created";
  if (!mkdir_p(d) || !jit_dir_trusted(d, &why))
    return fail(QIP_ERR_INVALID, "cache directory %s is not used: %s (code objects found there are loaded onto the GPU: the directory must belong to this user and be writable by nobody else)", dir, why.c_str());
  g_jit_dir = d;
  g_jit_dir_resolved = true;
  return QIP_OK;
} QIP_CATCH_ALL
extern "C" const char* qip_hip_jit_cache_dir(void) {
  static thread_local std::string out;
  try {
    std::lock_guard<std::mutex> lock(g_jit_mutex);
    out = g_jit_disk ? jit_dir_locked() : std::string();
  } catch (...) {
    return "";
  }
  return out.c_str();
}

extern "C" int qip_hip_jit_cache_info(uint64_t* resident, uint64_t* evicted, uint64_t* cap) try {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  if (resident) *resident = g_jit_cache.size();
  if (evicted) *evicted = g_jit_evictions;
  if (cap) *cap = (uint64_t)g_jit_cache_cap;
  return QIP_OK;
} QIP_CATCH_ALL

int jit_set_cache_cap(int64_t cap) {
  if (cap < 1) return fail(QIP_ERR_INVALID, "jit_cache_cap must be >= 1");
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  g_jit_cache_cap = cap;
  return QIP_OK;
}
uint64_t jit_cache_generation() {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  return g_jit_generation;
}

// under g_jit_mutex: unload least recently used kernels until the cache is within its bound
static void jit_evict_locked() {
  while ((int64_t)g_jit_cache.size() > g_jit_cache_cap) {
    auto victim = g_jit_cache.begin();
    for (auto it = g_jit_cache.begin(); it != g_jit_cache.end(); ++it)
      if (it->second.last_use < victim->second.last_use) victim = it;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(victim->second.device);
    (void)hipDeviceSynchronize();  // no launch of it may still be queued
    (void)hipModuleUnload(victim->second.module);
    (void)hipSetDevice(cur);
    g_jit_cache.erase(victim);
    g_jit_evictions += 1;
    g_jit_generation += 1;
  }
}

// ---- from a job to a code object -------------------------------------------------------------------------------------------------
// What one pass over some jobs counted: gathered without a lock, added to the counters in one step.
struct JitTally {
  uint64_t hits = 0, compiled_here = 0, stored = 0, by_helpers = 0, helper_procs = 0;
  double load_ms = 0, compile_ms = 0;
};
// under g_jit_mutex
static void jit_count_locked(const std::string& dir, const JitTally& t) {
  g_jit_disk_hits += t.hits;
  g_jit_load_ms += t.load_ms;
  g_jit_helper_procs += t.helper_procs;
  g_jit_helper_segments += t.by_helpers;
  g_jit_compiles += t.compiled_here + t.by_helpers;
  g_jit_disk_stores += t.stored + t.by_helpers;
  g_jit_compile_ms += t.compile_ms;
  if (t.stored + t.by_helpers) jit_disk_trim(dir);
}
// under g_jit_mutex: the directory in use ("" = none: no directory, or option "jit_disk_cache" = 0)
static std::string jit_disk_dir_locked() { return g_jit_disk ? jit_dir_locked() : std::string(); }

// A job's place in the disk cache (`dir` not empty): its key and file name — kept for the later store — and, on a hit, its code object.
struct JitDiskSlot {
  JitHash h;
  std::string path;
};
static bool jit_disk_lookup(const std::string& dir, const JitJob& job, JitDiskSlot* at, std::vector<char>* code, JitTally* t) {
  if (dir.empty()) return false;
  at->h = jit_hash(job.src, job.fma);
  at->path = jit_disk_path(dir, at->h);
  const auto t0 = std::chrono::steady_clock::now();
  if (!jit_disk_read(at->path, job.src.size(), at->h, code)) return false;
  t->load_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  t->hits += 1;
  return true;
}
// Compile one job in this process and store the code object at its place (`at`: from the lookup that missed).
static int jit_compile_here(const std::string& dir, const JitJob& job, const JitDiskSlot& at, std::vector<char>* code, JitTally* t) {
  const auto t0 = std::chrono::steady_clock::now();
  QCHK(hiprtc_compile(job.src, job.fma, code));
  t->compile_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  t->compiled_here += 1;
  if (!dir.empty() && jit_disk_write(at.path, job.src.size(), at.h, *code)) t->stored += 1;
  return QIP_OK;
}
// the same segment twice in one plan: once
static void jit_dedup(std::vector<JitJob>* jobs) {
  std::vector<JitJob> uniq;
  for (JitJob& j : *jobs)
    if (std::find(uniq.begin(), uniq.end(), j) == uniq.end()) uniq.push_back(std::move(j));
  jobs->swap(uniq);
}

// Device-free half: the code objects of `jobs` — from the disk cache, from helper processes, or compiled here.
int jit_obtain_code(const std::vector<JitJob>& jobs, std::vector<std::vector<char>>* code_out) {
  const size_t nj = jobs.size();
  if (const char* dump = getenv("QIP_HIP_JIT_DUMP_DIR")) {  // debugging aid (tools/jit_segment_resources.py): every segment's source, numbered
    static std::atomic<unsigned> serial{0};
    if (*dump && mkdir_p(dump))
      for (size_t i = 0; i < nj; ++i) {
        char name[64];
        snprintf(name, sizeof name, "/seg_%04u%s.hip", serial.fetch_add(1), jobs[i].fma ? "_fma" : "");
        if (FILE* f = fopen((std::string(dump) + name).c_str(), "wb")) {
          (void)fwrite(jobs[i].src.data(), 1, jobs[i].src.size(), f);
          fclose(f);
        }
      }
  }
  std::vector<std::vector<char>>& code = *code_out;
  code.assign(nj, std::vector<char>());
  std::string dir;
  int procs = 1;
  {
    std::lock_guard<std::mutex> lock(g_jit_mutex);
    dir = jit_disk_dir_locked();
    procs = jit_procs_effective();
  }
  // 1. what the disk cache already holds
  JitTally t;
  std::vector<JitDiskSlot> at(nj);
  std::vector<size_t> todo;
  for (size_t i = 0; i < nj; ++i)
    if (!jit_disk_lookup(dir, jobs[i], &at[i], &code[i], &t)) todo.push_back(i);
  // 2. the rest: side by side in helper processes when there are several (and somewhere to put the results) ...
  // (a process with a foreign libhiprtc sends single segments out too — unless "jit_procs" = 1 asks for this process only)
  if (!todo.empty() && !dir.empty() && ((todo.size() >= 2 && procs > 1) || (g_jit_procs != 1 && jit_foreign_hiprtc_loaded()))) {
    const std::string helper = jit_helper_path();
    if (!helper.empty()) {
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<std::string> paths(nj);
      for (size_t i : todo) paths[i] = at[i].path;
      t.helper_procs = jit_spawn_helpers(helper, dir, (size_t)procs, jobs, todo, paths, false);
      std::vector<size_t> still;
      for (size_t i : todo) {
        if (jit_disk_read(at[i].path, jobs[i].src.size(), at[i].h, &code[i])) t.by_helpers += 1;
        else still.push_back(i);
      }
      todo.swap(still);
      t.compile_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  // 3. ... and whatever is left (no helper, a single segment, a helper that failed: the message comes from here) in this process
  for (size_t i : todo) QCHK(jit_compile_here(dir, jobs[i], at[i], &code[i], &t));
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  jit_count_locked(dir, t);
  return QIP_OK;
}

// ---- from a code object to a resident kernel -------------------------------------------------------------------------------------
static std::string jit_key(const qip_hip_state* s, const JitJob& job) {
  return std::to_string(s->device) + (job.fma ? " fma\n" : "\n") + job.src;
}
// under g_jit_mutex: a compiled code object becomes a resident kernel of the cache
static int jit_insert_locked(qip_hip_state* s, const std::string& key, const std::vector<char>& code) {
  JitKernel k;
  HIPCHK(hipModuleLoadData(&k.module, code.data()));
  hipError_t e = hipModuleGetFunction(&k.fn, k.module, "qip_segment");
  if (e != hipSuccess) {
    (void)hipModuleUnload(k.module);
    return fail(QIP_ERR_DEVICE, "hipModuleGetFunction failed: %s", hipGetErrorString(e));
  }
  k.device = s->device;
  k.last_use = ++g_jit_clock;
  g_jit_loaded += 1;
  g_jit_cache[key] = k;
  return QIP_OK;
}
// under g_jit_mutex: the code objects of `n` jobs become resident kernels — unless another thread's handle got there first — and the
// cache returns to its bound (never at the cost of the entry inserted last: it is the most recently used).  Nothing is evicted
// while a graph is being recorded: unloading synchronises the device, which a capture forbids; the cache overshoots its bound until
// the next ordinary call.
static int jit_make_resident_locked(qip_hip_state* s, const JitJob* jobs, const std::vector<char>* code, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const std::string key = jit_key(s, jobs[i]);
    if (g_jit_cache.find(key) == g_jit_cache.end()) QCHK(jit_insert_locked(s, key, code[i]));
  }
  if (!s->capture_pool && g_jit_captures_in_progress == 0) jit_evict_locked();
  return QIP_OK;
}

// Look the job's kernel up (compile it on a miss) and — unless `launch` is null (compile-only pass before a graph capture) —
// launch it, all under the cache's mutex: between "here is the function" and "it is enqueued" no other thread may evict and
// unload it.  (Launches are asynchronous: the critical section is microseconds on a hit.)
// `collect` (a compile-only pass, BatchRun::jit_collect): a miss without `launch` is collected there instead of compiled.
int jit_run(qip_hip_state* s, const JitJob& job, const std::function<int(hipFunction_t)>& launch, std::vector<JitJob>* collect) {
  const std::string key = jit_key(s, job);
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  auto it = g_jit_cache.find(key);
  if (it != g_jit_cache.end()) {
    it->second.last_use = ++g_jit_clock;
  } else {
    if (!launch && collect) {
      collect->push_back(job);  // (the pre-compilation of a plan: jit_prepare)
      return QIP_OK;
    }
    // from the disk cache, or compiled here (and then stored there)
    const std::string dir = jit_disk_dir_locked();
    JitTally t;
    JitDiskSlot at;
    std::vector<char> code;
    if (!jit_disk_lookup(dir, job, &at, &code, &t)) QCHK(jit_compile_here(dir, job, at, &code, &t));
    jit_count_locked(dir, t);
    QCHK(jit_make_resident_locked(s, &job, &code, 1));
    it = g_jit_cache.find(key);
  }
  return launch ? launch(it->second.fn) : QIP_OK;
}
// Launch what was recorded under generation `gen` — a hipGraph that names resident kernels — unless the cache has evicted since
// (`*stale`, nothing runs): check and launch in ONE critical section, an eviction on another thread between the two would unload a
// module the graph names.  Enqueueing is asynchronous: the section is microseconds.
int jit_launch_if_current(uint64_t gen, const std::function<int()>& launch, bool* stale) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  *stale = gen != g_jit_generation;
  return *stale ? QIP_OK : launch();
}

// Every job of a plan made resident before anything runs: found in the disk cache, the rest compiled side by side in helper
// processes (jit_obtain_code).
int jit_prepare(qip_hip_state* s, std::vector<JitJob>& jobs) {
  jit_dedup(&jobs);
  if (jobs.empty()) return QIP_OK;
  std::vector<std::vector<char>> code;
  QCHK(jit_obtain_code(jobs, &code));
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  return jit_make_resident_locked(s, jobs.data(), code.data(), jobs.size());
}

// ---- r6: compiled sweeps for one-shot callers, when they are free (option "tile_auto") -------------------------------------
// apply_ops on a state with tile >= 1 and tile_jit = 0 is what a `calculate_state` caller issues (HipBuilder): once.  It does not
// repay seconds of compilation — but a plan whose segments are ALL already resident or in the disk cache costs milliseconds to
// load and runs 1.5x faster than the interpreter.  So such a call LOOKS its wide plan up (jit_lookup): all hits -> compiled
// sweeps (bit-identical to the interpreter for tile = 1); any miss -> the interpreter runs now, and the missing segments are
// handed to helper processes nobody waits for (jit_compile_in_background): the next call, or the next process, finds them.
static std::map<std::string, std::chrono::steady_clock::time_point> g_jit_inflight;  // object paths handed to background helpers

// the jobs that are resident or on disk become resident; the others are returned in `misses` (nothing is compiled)
int jit_lookup(qip_hip_state* s, std::vector<JitJob>& jobs, std::vector<JitJob>* misses) {
  jit_dedup(&jobs);
  std::string dir;
  {
    std::lock_guard<std::mutex> lock(g_jit_mutex);
    dir = jit_disk_dir_locked();
  }
  std::vector<std::vector<char>> code(jobs.size());
  JitTally t;
  for (size_t i = 0; i < jobs.size(); ++i) {
    JitDiskSlot at;
    if (!jit_disk_lookup(dir, jobs[i], &at, &code[i], &t)) misses->push_back(jobs[i]);
  }
  if (!misses->empty()) return QIP_OK;  // (a partial plan is of no use: nothing is counted, nothing is loaded onto the device)
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  jit_count_locked(dir, t);
  return jit_make_resident_locked(s, jobs.data(), code.data(), jobs.size());
}

// Hand `jobs` to helper processes and return at once: they write the code objects into the disk cache.  Jobs handed out less
// than two minutes ago are not handed out again.
void jit_compile_in_background(const std::vector<JitJob>& jobs) {
  std::string dir;
  int procs = 1;
  std::vector<size_t> todo;
  std::vector<std::string> out_paths(jobs.size());
  {
    std::lock_guard<std::mutex> lock(g_jit_mutex);
    dir = jit_disk_dir_locked();
    if (dir.empty()) return;  // nowhere to leave the results
    procs = jit_procs_effective();
    const auto now = std::chrono::steady_clock::now();
    for (auto it = g_jit_inflight.begin(); it != g_jit_inflight.end();)
      it = now - it->second > std::chrono::seconds(120) ? g_jit_inflight.erase(it) : std::next(it);
    for (size_t i = 0; i < jobs.size(); ++i) {
      out_paths[i] = jit_disk_path(dir, jit_hash(jobs[i].src, jobs[i].fma));
      if (g_jit_inflight.count(out_paths[i])) continue;
      g_jit_inflight[out_paths[i]] = now;
      todo.push_back(i);
    }
    g_jit_background_segments += todo.size();
  }
  if (todo.empty()) return;
  const std::string helper = jit_helper_path();
  if (helper.empty()) return;
  // (half of the usual share: the caller's own sweeps are running on this host's cores' attention too)
  const size_t spawned = jit_spawn_helpers(helper, dir, (size_t)std::max(1, procs / 2), jobs, todo, out_paths, true);
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  g_jit_helper_procs += spawned;
}

// ---- the plan memo -----------------------------------------------------------------------------------------------------------------
// A plan that has had all its segments made resident is remembered by a fingerprint of its structure (the caller's: it walks the
// plan), so the steady state — the same circuit applied again and again — does not generate every source twice; a plan that a
// lookup-only pass found incomplete is remembered too: its segments are still being compiled, do not look again yet.
static std::set<uint64_t> g_jit_warm_plans;  // fingerprints of plans whose segments have all been made resident (apply_ops_tiled)
static uint64_t g_jit_warm_generation = 0;   // ... as long as nothing has been evicted since
static std::map<uint64_t, std::chrono::steady_clock::time_point> g_jit_cold_plans;  // plan fingerprints last seen incomplete
JitPlanMemo jit_plan_query(uint64_t fp) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  if (g_jit_warm_plans.count(fp) != 0 && g_jit_warm_generation == g_jit_generation) return JitPlanMemo::kWarm;
  auto it = g_jit_cold_plans.find(fp);
  const bool recent = it != g_jit_cold_plans.end() && std::chrono::steady_clock::now() - it->second < std::chrono::milliseconds(1500);
  return recent ? JitPlanMemo::kColdRecently : JitPlanMemo::kUnknown;
}
void jit_plan_mark_warm(uint64_t fp) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  if (g_jit_warm_generation != g_jit_generation || g_jit_warm_plans.size() > 4096) {  // (an eviction may have dropped what a warm plan needs)
    g_jit_warm_plans.clear();
    g_jit_warm_generation = g_jit_generation;
  }
  g_jit_warm_plans.insert(fp);
}
void jit_plan_mark_cold(uint64_t fp) {
  std::lock_guard<std::mutex> lock(g_jit_mutex);
  if (g_jit_cold_plans.size() > 1024) g_jit_cold_plans.clear();
  g_jit_cold_plans[fp] = std::chrono::steady_clock::now();
}
