// mock_library.cpp - the library's translation unit linked against the model of the HIP runtime (tests/mock_hip.hpp) as a shared object:
// the Python layer (ctypes table, CsiEngine, pinned result pool) then runs on a machine without a GPU.  Kernel launches are dropped, so
// numbers are meaningless - call flow, argument checks, buffer lifetimes and counters are what it serves (tests/test_host_round4.py).
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -shared -fPIC -pthread tests/mock_library.cpp -o /tmp/libcsi_mock.so
#include "../dl-channel-estimation-mamimo_amd/csrc/csi_mamimo.hip"

#include "mock_hip.hpp"

// ---- which band kernel served a call (tests/test_band_routes_host.py): one text line per module launch whose argument record is a
// Band8Args (128 bytes) or a Band8ArgsCs (144 bytes) -
//   <kernel name> grid=<x>,<y> block=<x> bytes=<record> M=<> N1=<> nt=<> tiled=<1 tiled copy | 0 plain weights | ?> [part=<0 | 1>]
// The record's W1 is kept and named when the log is read: a model's tiled copy (Model::Wt1) is allocated once and stays.
// Test-only entry points of THIS translation unit; the product header does not know them.
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
}  // namespace

extern "C" {
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
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>(text.size(), (size_t)cap - 1);
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int64_t)text.size() + 1;
}
void csi_mock_band_log_clear(void) {
    std::lock_guard<std::mutex> lk(band_log_mu);
    band_log.clear();
}
}  // extern "C"
#endif
