// mock_library.cpp - the library's translation unit linked against the model of the HIP runtime (tests/mock_hip.hpp) as a shared object:
// the Python layer (ctypes table, CsiEngine, pinned result pool) then runs on a machine without a GPU.  Kernel launches are dropped, so
// numbers are meaningless - call flow, argument checks, buffer lifetimes and counters are what it serves (tests/test_host_round4.py).
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -shared -fPIC -pthread tests/mock_library.cpp -o /tmp/libcsi_mock.so
#include "../dl-channel-estimation-mamimo_amd/csrc/csi_mamimo.hip"

#include "mock_hip.hpp"
#include <cxxabi.h>
#include <dlfcn.h>

// ---- which band kernel served a call (tests/test_band_routes_host.py): one text line per module launch whose argument record is a
// Band8Args (128 bytes) or a Band8ArgsCs (144 bytes) -
//   <kernel name> grid=<x>,<y> block=<x> bytes=<record> M=<> N1=<> nt=<> tiled=<1 tiled copy | 0 plain weights | ?> [part=<0 | 1>]
// The record's W1 is kept and named when the log is read: a model's tiled copy (Model::Wt1) is allocated once and stays.
// Test-only entry points of THIS translation unit; the product header does not know them.  (Further down: the log of the LS kernels and the log of the staged host calls.)
#if !defined(__HIP_DEVICE_COMPILE__)
namespace {
struct BandLaunch { std::string name; unsigned gx, gy, bx; size_t bytes; Band8ArgsCs rec; };
std::mutex band_log_mu;
std::vector<BandLaunch> band_log;
const bool band_log_hooked = [] {
    mock::module_launch_hook = [](const char* name, unsigned gx, unsigned gy, unsigned bx, const void* params, size_t bytes, hipStream_t) {
        if (!params || (bytes != sizeof(Band8Args) && bytes != sizeof(Band8ArgsCs))) return;
        BandLaunch l{name, gx, gy, bx, bytes, {}};
        std::memcpy(&l.rec, params, bytes);
        std::lock_guard<std::mutex> lk(band_log_mu);
        band_log.push_back(l);
    };
    return true;
}();

// ---- which LS kernel served a call, and what csi_set_pilot uploaded (tests/test_ls_routes_host.py).  One text line per
// hipFuncSetAttribute and per hipLaunchKernel of an LS kernel -
//   attr value=<bytes> kernel=<name>
//   launch grid=<x>,<y> block=<x> lds=<dynamic bytes> attr=<1: the last attribute line names this kernel and these bytes | 0> kernel=<name>
// <name> is what the dynamic linker knows the kernel's host handle by, demangled, without the return type and the namespace:
// "ls_estimate_ring_kernel<1, 4, 8, 1, 3>(csi::LsArgs, int)".  Kernels whose name does not start with ls_ or small_l0_ls_kernel stay out.
std::mutex ls_log_mu;
std::vector<std::string> ls_log;
const void* ls_attr_fn = nullptr;
int ls_attr_value = -1;
std::string kernel_name(const void* fn) {
    Dl_info info{};
    if (!dladdr(fn, &info) || !info.dli_sname || info.dli_saddr != fn) return "";
    int status = 0;
    char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
    std::string s = status == 0 && d ? d : info.dli_sname;
    std::free(d);
    for (const char* prefix : {"void ", "csi::"})
        if (s.compare(0, std::strlen(prefix), prefix) == 0) s.erase(0, std::strlen(prefix));
    return s;
}
std::string ls_kernel_name(const void* fn) {
    const std::string s = kernel_name(fn);
    return s.compare(0, 3, "ls_") == 0 || s.compare(0, 18, "small_l0_ls_kernel") == 0 ? s : "";
}

// ---- what a staged host call does (tests/test_staged_calls_host.py).  While a context is named (csi_mock_stage_log_clear), one text line
// per hipMalloc, hipMemcpyAsync / hipMemcpy, hipLaunchKernel and hipStreamSynchronize of the process -
//   malloc bytes=<requested>
//   copy <H2D | D2H | ...> bytes=<> dev=<buffer>+<offset> host=<array>+<offset>
//   launch grid=<x>,<y>,<z> block=<x>,<y>,<z> lds=<dynamic bytes> kernel=<name as in the LS log, every kernel>
//   sync
// <buffer> is the context's buffer that holds the device address (stage, skbuf, ...: stage_log_where), <array> the host array the test
// named (csi_mock_stage_log_name) that holds the host address; "local" is an address none of them holds (a variable of the library's).
std::mutex stage_log_mu;
std::vector<std::string> stage_log;
csi_ctx* stage_log_ctx = nullptr;
struct NamedRange { std::string name; const char* base; size_t bytes; };
std::vector<NamedRange> stage_log_arrays;
std::string stage_log_where(const void* p, bool device) {
    const char* a = static_cast<const char*>(p);
    const csi_ctx* c = stage_log_ctx;
    const size_t slack = G_SLACK_FLOATS * sizeof(float);      // ensure_bytes allocates it behind the bytes it was asked for
    std::vector<NamedRange> dev = {{"stage", c->stage, c->stage_bytes + slack}, {"skbuf", c->skbuf, c->skbuf_bytes + slack},
                                   {"lmb_ws", c->lmb_ws, c->lmb_ws_bytes + slack}, {"hyb_ws", c->hyb_ws, c->hyb_ws_bytes + slack},
                                   {"beam_ws", c->beam_ws, c->beam_ws_bytes + slack},
                                   {"sub_q", reinterpret_cast<const char*>(c->sub_q), SB_IMAGE_FLOATS * sizeof(float)},
                                   {"beam_a", reinterpret_cast<const char*>(c->beam_a), BM_IMAGE_FLOATS * sizeof(float)}};
    for (const NamedRange& r : device ? dev : stage_log_arrays)
        if (r.base && a >= r.base && a < r.base + r.bytes) return r.name + "+" + std::to_string(a - r.base);
    return "local";
}
const bool stage_log_hooked = [] {
    mock::alloc_hook = [](size_t bytes) {
        std::lock_guard<std::mutex> lk(stage_log_mu);
        if (stage_log_ctx) stage_log.push_back("malloc bytes=" + std::to_string(bytes));
    };
    mock::copy_hook = [](const void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        std::lock_guard<std::mutex> lk(stage_log_mu);
        if (!stage_log_ctx) return;
        const bool up = kind == hipMemcpyHostToDevice, down = kind == hipMemcpyDeviceToHost;
        if (!up && !down) { stage_log.push_back("copy kind=" + std::to_string((int)kind) + " bytes=" + std::to_string(bytes)); return; }
        stage_log.push_back(std::string("copy ") + (up ? "H2D" : "D2H") + " bytes=" + std::to_string(bytes) + " dev=" + stage_log_where(up ? dst : src, true) +
                      " host=" + stage_log_where(up ? src : dst, false));
    };
    mock::sync_hook = [](hipStream_t) {
        std::lock_guard<std::mutex> lk(stage_log_mu);
        if (stage_log_ctx) stage_log.push_back("sync");
    };
    return true;
}();
const bool ls_log_hooked = [] {
    mock::func_attribute_hook = [](const void* fn, hipFuncAttribute attr, int value) {
        const std::string name = ls_kernel_name(fn);
        if (name.empty() || attr != hipFuncAttributeMaxDynamicSharedMemorySize) return;
        std::lock_guard<std::mutex> lk(ls_log_mu);
        ls_attr_fn = fn;
        ls_attr_value = value;
        ls_log.push_back("attr value=" + std::to_string(value) + " kernel=" + name);
    };
    mock::launch_shape_hook = [](const void* fn, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t) {
        {
            std::lock_guard<std::mutex> lk(stage_log_mu);
            if (stage_log_ctx) {
                char line[160];
                std::snprintf(line, sizeof line, "launch grid=%u,%u,%u block=%u,%u,%u lds=%zu kernel=", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds_bytes);
                stage_log.push_back(line + kernel_name(fn));
            }
        }
        const std::string name = ls_kernel_name(fn);
        if (name.empty()) return;
        std::lock_guard<std::mutex> lk(ls_log_mu);
        char line[160];
        std::snprintf(line, sizeof line, "launch grid=%u,%u block=%u lds=%zu attr=%d kernel=", grid.x, grid.y, block.x, lds_bytes,
                      fn == ls_attr_fn && (size_t)ls_attr_value == lds_bytes);
        ls_log.push_back(line + name);
    };
    return true;
}();
int64_t text_out(const std::string& text, char* buf, int64_t cap) {
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>(text.size(), (size_t)cap - 1);
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int64_t)text.size() + 1;
}
}  // namespace

extern "C" {
// the LS log as text into buf (at most cap bytes incl. the terminator); returns the bytes the whole text needs
int64_t csi_mock_ls_log_read(char* buf, int64_t cap) {
    std::string text;
    std::lock_guard<std::mutex> lk(ls_log_mu);
    for (const std::string& l : ls_log) text += l + '\n';
    return text_out(text, buf, cap);
}
void csi_mock_ls_log_clear(void) {
    std::lock_guard<std::mutex> lk(ls_log_mu);
    ls_log.clear();
}
// the staged-call log: csi_mock_stage_log_clear empties it and names the context whose calls are kept from now on (null: none - before the
// context goes); csi_mock_stage_log_name names a host array (null name: forgets them all); csi_mock_stage_log_read as csi_mock_ls_log_read
void csi_mock_stage_log_clear(csi_ctx* c) {
    std::lock_guard<std::mutex> lk(stage_log_mu);
    stage_log.clear();
    stage_log_ctx = c;
}
void csi_mock_stage_log_name(const char* name, const void* base, int64_t bytes) {
    std::lock_guard<std::mutex> lk(stage_log_mu);
    if (!name) stage_log_arrays.clear();
    else stage_log_arrays.push_back({name, static_cast<const char*>(base), (size_t)bytes});
}
int64_t csi_mock_stage_log_read(char* buf, int64_t cap) {
    std::string text;
    std::lock_guard<std::mutex> lk(stage_log_mu);
    for (const std::string& l : stage_log) text += l + '\n';
    return text_out(text, buf, cap);
}
// what csi_set_pilot left on the "device" (host memory here): which = 0 P, 1 Ppad, 2 Pbf, 3 p_tables; returns the payload bytes (without the
// slack behind them; 0: the context has no such buffer) and the address in *ptr.  The sizes are written out here, not taken from the library.
int64_t csi_mock_pilot_buffer(csi_ctx* c, int which, const void** ptr) {
    const size_t nt = (size_t)c->cfg.nt, jt = (nt + 31) / 32, nch = (nt + 15) / 16;
    const void* p[4] = {c->P, c->Ppad, c->Pbf, c->p_tables};
    const size_t bytes[4] = {nt * nt * 4, jt * 32 * jt * 32 * 4, (nch * 3 * jt * 512 + 1) / 2 * 4, 4 * nt * 4};
    if (which < 0 || which > 3 || !p[which]) return 0;
    *ptr = p[which];
    return (int64_t)bytes[which];
}
// what csi_load_weights left on the "device" (tests/test_weight_prep_host.py): the index-th buffer of the loaded models in the order of
// wire_blobs, the pilot buffers left out; returns its bytes WITH the slack behind the payload (-1: no such buffer) and the address in *ptr
int64_t csi_mock_weight_blob(csi_ctx* c, int index, const void** ptr) {
    WireMeta w;
    wire_fill(c, w);
    w.pilot_ok = 0;
    std::vector<WBlob> blobs;
    wire_blobs(c, w, blobs);
    if (index < 0 || index >= (int)blobs.size()) return -1;
    *ptr = *blobs[index].p;
    return (int64_t)blobs[index].bytes;
}
// the record wire_fill makes of the context - every host-side scalar of the loaded models - into buf; returns the bytes it needs
int64_t csi_mock_wire_meta(csi_ctx* c, void* buf, int64_t cap) {
    WireMeta w;
    wire_fill(c, w);
    if (buf && cap >= (int64_t)sizeof w) std::memcpy(buf, &w, sizeof w);
    return (int64_t)sizeof w;
}
int64_t csi_mock_live_allocs(void) { return mock::g_live; }      // hipMalloc'ed buffers of the process not yet freed
// the log as text into buf (at most cap bytes incl. the terminator); returns the bytes the whole text needs
int64_t csi_mock_band_log_read(csi_ctx* c, char* buf, int64_t cap) {
    std::string text;
    std::lock_guard<std::mutex> lk(band_log_mu);
    for (const BandLaunch& l : band_log) {
        const char* tiled = "?";
        for (const Model& m : c->model) {
            if (m.layers.size() < 2) continue;
            if (m.Wt1 && l.rec.a.W1 == m.Wt1) tiled = "1";
            else if (l.rec.a.W1 == m.layers[1].Wh || l.rec.a.W1 == reinterpret_cast<const uint16_t*>(m.layers[1].Wb)) tiled = "0";
        }
        char line[256];
        int n = std::snprintf(line, sizeof line, "%s grid=%u,%u block=%u bytes=%zu M=%d N1=%d nt=%d tiled=%s", l.name.c_str(), l.gx, l.gy, l.bx, l.bytes,
                              l.rec.a.M, l.rec.a.N1, l.rec.a.nt, tiled);
        if (l.bytes == sizeof(Band8ArgsCs)) n += std::snprintf(line + n, sizeof line - n, " part=%d", l.rec.part != nullptr);
        text += line;
        text += '\n';
    }
    return text_out(text, buf, cap);
}
void csi_mock_band_log_clear(void) {
    std::lock_guard<std::mutex> lk(band_log_mu);
    band_log.clear();
}
}  // extern "C"
#endif
