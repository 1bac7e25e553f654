// Query compiler, compile + caches: the hipRTC compile of a generated source
// with its on-disk code objects, the in-memory module cache, and the shape
// fast path that finds a query shape's kernel without generating its source.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "jit_gen.h"

namespace dfmi {
namespace jit {

// ------------------------------------------------------------ compile cache
// Loaded code objects, keyed by device + source text, bounded (least recently
// used evicted past the cap). A module is unloaded when the last holder lets
// go: the cache, and every Launch that got its kernel from get_kernel
// (Launch::module) -- so a launch in flight keeps its code object loaded.
// The map itself is never destroyed: modules still cached at process exit
// are left to the runtime's teardown, as before the bound.
namespace {
struct Compiled {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    ~Compiled() {
        if (mod) (void)hipModuleUnload(mod);
    }
};
struct CacheEntry {
    std::shared_ptr<Compiled> c;
    uint64_t used = 0;
};
std::mutex g_mu;
auto& g_cache = *new std::map<std::string, CacheEntry>();  // guarded by g_mu
uint64_t g_tick = 0;
size_t g_cap = [] {
    const char* e = getenv("DFMI_JIT_CACHE_MODULES");
    return e && atoi(e) > 0 ? (size_t)atoi(e) : (size_t)256;
}();
// caller holds g_mu
void evict_to(size_t cap) {
    while (g_cache.size() > cap) {
        auto lru = g_cache.begin();
        for (auto it = g_cache.begin(); it != g_cache.end(); ++it)
            if (it->second.used < lru->second.used) lru = it;
        g_cache.erase(lru);
    }
}
}  // namespace

// ------------------------------------------------------- on-disk code objects
// A process's first call of a query shape would pay the hipRTC compile
// (~190 ms); the reference's compile_scalar_expr is a closure build
// (context.rs:131,152-155). Code objects are therefore also kept on disk,
// keyed by a hash of the generated source, the compile options, the hipRTC
// version and the target: DFMI_JIT_CACHE_DIR (empty: off), else
// $XDG_CACHE_HOME/dfmi-jit, else $HOME/.cache/dfmi-jit. A file holds the full
// source it was compiled from and is used only when that source matches
// byte for byte (a hash collision cannot load the wrong code); files are
// written to a temporary name and renamed, so a reader never sees a partial
// one, and a damaged or foreign file is ignored (compiled again).
namespace {
const char* const kOpts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17",
                             "-Wno-unused-variable", "-Wno-unused-but-set-variable"};

const std::string& disk_dir() {
    static const std::string dir = [] {
        std::string d;
        if (const char* e = getenv("DFMI_JIT_CACHE_DIR")) {
            d = e;  // "" disables
        } else if (const char* x = getenv("XDG_CACHE_HOME"); x && *x) {
            d = std::string(x) + "/dfmi-jit";
        } else if (const char* h = getenv("HOME"); h && *h) {
            d = std::string(h) + "/.cache/dfmi-jit";
        }
        if (!d.empty()) {  // mkdir -p
            for (size_t i = 1; i <= d.size(); ++i)
                if (i == d.size() || d[i] == '/') (void)::mkdir(d.substr(0, i).c_str(), 0755);
            struct stat st;
            if (::stat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) d.clear();
        }
        return d;
    }();
    return dir;
}

std::string disk_path(const std::string& src) {
    int maj = 0, min = 0;
    hiprtcVersion(&maj, &min);
    std::string salt = "dfmi-co-1 hiprtc " + std::to_string(maj) + "." + std::to_string(min);
    for (const char* o : kOpts) salt += std::string(" ") + o;
    uint64_t h1 = fnv1a(salt.data(), salt.size());
    h1 = fnv1a(src.data(), src.size(), h1);
    uint64_t h2 = fnv1a(src.data(), src.size(), 0x84222325cbf29ce4ull ^ src.size());
    h2 = fnv1a(salt.data(), salt.size(), h2);
    char name[64];
    snprintf(name, sizeof name, "/%016llx%016llx.co", (unsigned long long)h1, (unsigned long long)h2);
    return disk_dir() + name;
}

constexpr char kMagic[8] = {'D', 'F', 'M', 'I', 'C', 'O', '1', '\n'};

bool disk_load(const std::string& path, const std::string& src, std::vector<char>& code) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    bool ok = false;
    char magic[8];
    uint64_t ns = 0, nc = 0;
    if (fread(magic, 1, 8, f) == 8 && !memcmp(magic, kMagic, 8) && fread(&ns, 8, 1, f) == 1 && ns == src.size()) {
        std::string s(ns, '\0');
        if (fread(&s[0], 1, ns, f) == ns && s == src && fread(&nc, 8, 1, f) == 1 && nc > 0 && nc < ((uint64_t)1 << 30)) {
            code.resize(nc);
            ok = fread(code.data(), 1, nc, f) == nc && fgetc(f) == EOF;
        }
    }
    fclose(f);
    return ok;
}

void disk_store(const std::string& path, const std::string& src, const std::vector<char>& code) {
    char tmp[64];
    snprintf(tmp, sizeof tmp, ".tmp.%d.%llx", (int)getpid(),
             (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count());
    const std::string t = path + tmp;
    FILE* f = fopen(t.c_str(), "wb");
    if (!f) return;
    const uint64_t ns = src.size(), nc = code.size();
    bool ok = fwrite(kMagic, 1, 8, f) == 8 && fwrite(&ns, 8, 1, f) == 1 && fwrite(src.data(), 1, ns, f) == ns &&
              fwrite(&nc, 8, 1, f) == 1 && fwrite(code.data(), 1, nc, f) == nc;
    ok = fclose(f) == 0 && ok;
    if (!ok || ::rename(t.c_str(), path.c_str()) != 0) ::unlink(t.c_str());
}
}  // namespace

std::vector<char> compile_code(const std::string& src, double* compile_ms) {
    if (compile_ms) *compile_ms = 0;
    std::string path;
    if (!disk_dir().empty()) {
        path = disk_path(src);
        std::vector<char> code;
        if (disk_load(path, src, code)) return code;  // no compile: *compile_ms stays 0
    }
    std::vector<char> code = compile_code_rtc(src, compile_ms);
    if (!path.empty()) disk_store(path, src, code);
    return code;
}

std::vector<char> compile_code_rtc(const std::string& src, double* compile_ms) {
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "dfmi_query.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        throw Fail{DFMI_ERR_DEVICE, "hiprtcCreateProgram failed"};
    const auto t0 = std::chrono::steady_clock::now();
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof kOpts / sizeof *kOpts), kOpts);
    if (compile_ms)
        *compile_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, '\0');
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        if (getenv("DFMI_JIT_DUMP")) fprintf(stderr, "%s\n----\n%s\n", src.c_str(), log.c_str());
        throw Fail{DFMI_ERR_DEVICE, "query compile failed: " + log.substr(0, 400)};
    }
    size_t size = 0;
    hiprtcGetCodeSize(prog, &size);
    std::vector<char> code(size);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    return code;
}

static std::shared_ptr<Compiled> compile(int device, const std::string& src, const std::string& name,
                                         double* compile_ms) {
    const std::string key = std::to_string(device) + "\n" + src;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_cache.find(key);
    if (it != g_cache.end()) {
        it->second.used = ++g_tick;
        return it->second.c;
    }
    const std::vector<char> code = compile_code(src, compile_ms);
    auto c = std::make_shared<Compiled>();
    if (hipModuleLoadData(&c->mod, code.data()) != hipSuccess) {
        c->mod = nullptr;
        throw Fail{DFMI_ERR_DEVICE, "hipModuleLoadData failed"};
    }
    if (hipModuleGetFunction(&c->fn, c->mod, name.c_str()) != hipSuccess)
        throw Fail{DFMI_ERR_DEVICE, "hipModuleGetFunction failed"};
    evict_to(g_cap - 1);
    g_cache[key] = CacheEntry{c, ++g_tick};
    return c;
}

size_t cache_size() {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_cache.size();
}

size_t cache_cap(size_t cap) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (cap > 0) {
        g_cap = cap;
        evict_to(cap);
    }
    return g_cap;
}

// ------------------------------------------------------- shape fast path
// A call whose programs, batch column types / nullability and tile shape
// match an earlier call launches the same kernel with the same literal
// tables: programs are immutable and carry a never-reused uid, so the key
// below identifies the generated source without generating it (~20 KB of
// text per call otherwise).
namespace {
struct ShapeHit {
    std::weak_ptr<Compiled> mod;  // an evicted module makes the entry stale
    std::string kname;
    LitPool lits;
};
std::unordered_map<std::string, ShapeHit> g_shapes;  // guarded by g_mu

template <typename T>
void put(std::string& k, const T& v) {
    k.append((const char*)&v, sizeof v);
}

std::string shape_key(int device, const Plan& P, const Launch& X) {
    std::string k;
    k.reserve(256);
    put(k, device);
    put(k, P.pred ? P.pred->uid : 0ull);
    put(k, P.gkey ? P.gkey->uid : 0ull);
    put(k, P.gkey_ord);
    put(k, P.gslots);
    for (const AggSpec& a : P.aggs) {
        put(k, a.fn);
        put(k, a.prog ? a.prog->uid : 0ull);
        put(k, a.ord_base);
        put(k, a.fslot);
    }
    for (const OutSpec& os : P.outs) {
        put(k, (int)os.kind);
        put(k, os.col);
        put(k, os.prog ? os.prog->uid : 0ull);
        put(k, os.ord_base);
        put(k, os.out_type);
        put(k, (char)os.nullable);
    }
    // every code-shaping knob, whole: a new one belongs in TileShape (jit.h)
    // and is then part of the key without a word here
    put(k, static_cast<const TileShape&>(X));
    for (int c : X.num_cols) {
        put(k, c);
        put(k, (char)X.col_type(c));
        put(k, (char)X.col_nullable(c));
    }
    put(k, (int)X.pred_slots.size());
    for (int c : X.utf8_cols) {
        put(k, c);
        put(k, (char)X.col_nullable(c));
    }
    for (const auto& uo : X.utf8_outs) {
        put(k, uo.first);
        put(k, uo.second);
    }
    return k;
}
}  // namespace

hipFunction_t get_kernel(int device, const Plan& P, Launch& X, double* compile_ms) {
    if (compile_ms) *compile_ms = 0;
    const std::string key = shape_key(device, P, X);
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_shapes.find(key);
        std::shared_ptr<Compiled> c;
        if (it != g_shapes.end() && !(c = it->second.mod.lock())) g_shapes.erase(it), it = g_shapes.end();
        if (it != g_shapes.end()) {
            const ShapeHit& h = it->second;
            X.module = c;
            X.lits = h.lits;
            X.kname = h.kname;
            return c->fn;
        }
    }
    std::string src = generate(P, X);
    if (getenv("DFMI_JIT_PRINT"))  // the generated body (after the skeleton)
        fprintf(stderr, "%s\n", src.c_str() + std::min(src.size(), src.find(skeleton_text()) + skeleton_text().size()));
    std::shared_ptr<Compiled> c = compile(device, src, X.kname, compile_ms);
    const bool soft = X.waves_soft && X.waves_per_eu > 0;
    // a soft occupancy hint: if the register allocator had to spill more
    // than a little to meet it, the query shape is compiled again without
    // it (the C3 gather kernel spills 72 B/lane under hipRTC at 8
    // waves/SIMD and is still 6% faster than at 6 waves)
    constexpr int kSoftSpill = 128;
    int scratch = 0, regs = 0;
    bool spills = false;
    if (soft || getenv("DFMI_JIT_VERBOSE")) {
        const bool got = hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, c->fn) == hipSuccess;
        (void)hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, c->fn);
        spills = soft && got && scratch > kSoftSpill;
        if (getenv("DFMI_JIT_VERBOSE"))  // (tools/*_probe.py read this line)
            fprintf(stderr, "dfmi jit: %s waves_per_eu %d: scratch %d B/lane, %d VGPRs%s\n", X.kname.c_str(),
                    X.waves_per_eu, scratch, regs, spills ? " -> recompiled without the hint" : "");
    }
    if (spills) {
        // (the entry below stays under the key with the hint: a later hit returns
        // this kernel while X.waves_per_eu reads 8 -- nothing reads it after get_kernel)
        double ms2 = 0;
        X.waves_per_eu = 0;
        src = generate(P, X);
        c = compile(device, src, X.kname, &ms2);
        if (compile_ms) *compile_ms += ms2;
    }
    X.module = c;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_shapes.size() >= 4096) g_shapes.clear();  // bounded: programs come and go
    g_shapes[key] = ShapeHit{c, X.kname, X.lits};
    return c->fn;
}

}  // namespace jit
}  // namespace dfmi
