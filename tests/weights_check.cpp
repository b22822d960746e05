// weights_check.cpp - csi_load_weights / csi_clone_weights / csi_destroy in a stand-alone program: the library's whole translation unit against
// the model of the HIP runtime (tests/mock_hip.hpp, "device" memory on the host).  Three contexts - the split-f16 engine with every copy of the
// regressor (Wh, Wh_f, Wh_p), a bf16 context with its band copy (Wb_p), a CONV1D model on a context with one hidden layer - are loaded (both
// component models), cloned into a second context and destroyed.  Checked: the clone holds the source's buffers byte for byte, slack included,
// with the sizes the buffer table (csi_context.hpp) gives; nothing stays allocated.  Its other purpose is a host sanitizer build, run directly:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -pthread -Xarch_host -fsanitize=address,undefined tests/weights_check.cpp -o /tmp/wc && /tmp/wc
// - the upload writes payload + slack of the table's sizes into allocations of the table's sizes, the clone copies them whole.
// Test scaffolding for OUR host code; not a stand-in for anything of the reference.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -pthread tests/weights_check.cpp -o /tmp/weights_check && /tmp/weights_check
#include "../dl-channel-estimation-mamimo_amd/csrc/csi_mamimo.hip"

#include "mock_hip.hpp"

#if !defined(__HIP_DEVICE_COMPILE__)
namespace {

struct Shape { int nt, n_hidden, hidden[3], n_out, dtype, conv; };

int bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++bad; std::printf("FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

csi_ctx* make_ctx(const Shape& s) {
    csi_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.nt = s.nt; cfg.nr = 2; cfg.len_ltf = 320 * s.nt; cfg.n_hidden = s.n_hidden;
    for (int i = 0; i < s.n_hidden; ++i) cfg.hidden[i] = s.hidden[i];
    cfg.n_out = s.n_out; cfg.use_bn = 1; cfg.bn_eps = 1e-3f; cfg.dtype = (csi_dtype)s.dtype;
    csi_ctx* c = nullptr;
    if (csi_create(&cfg, &c) != CSI_OK) { std::printf("csi_create: %s\n", csi_last_error(nullptr)); std::exit(3); }
    if (s.conv && csi_set_model_type(c, CSI_MODEL_CONV1D) != CSI_OK) { std::printf("csi_set_model_type: %s\n", csi_last_error(c)); std::exit(3); }
    return c;
}

int load(csi_ctx* c, const Shape& s, int model, unsigned seed) {
    std::deque<std::vector<float>> keep;
    std::deque<std::string> names;
    std::vector<csi_tensor> t;
    auto add = [&](const std::string& name, int rows, int cols) {
        keep.emplace_back((size_t)rows * cols);
        std::vector<float>& v = keep.back();
        const float lift = name.find("variance") != std::string::npos || name.find("gamma") != std::string::npos ? 1.f : 0.f;
        for (size_t i = 0; i < v.size(); ++i) v[i] = (float)((i * 2654435761u + seed) % 2003) / 2003.f - 0.5f + lift;
        names.push_back(name);
        t.push_back(csi_tensor{names.back().c_str(), v.data(), rows, cols});
    };
    if (s.conv) {
        add("cnn1d_1.kernel", CONV_TAPS, CONV_FILTERS);
        for (const char* k : {"cnn1d_1.bias", "conv_bn.gamma", "conv_bn.beta", "conv_bn.moving_mean", "conv_bn.moving_variance"}) add(k, 1, CONV_FILTERS);
    }
    int in = (s.conv ? 64 * 320 : 320) * s.nt + s.nt;
    for (int l = 0; l < s.n_hidden; ++l) {
        add("fc_dense" + std::to_string(l) + ".kernel", in, s.hidden[l]);
        add("fc_dense" + std::to_string(l) + ".bias", 1, s.hidden[l]);
        for (const char* k : {".gamma", ".beta", ".moving_mean", ".moving_variance"}) add("bn" + std::to_string(l) + k, 1, s.hidden[l]);
        in = s.hidden[l];
    }
    add("fc_regressor.kernel", in, s.n_out);
    add("fc_regressor.bias", 1, s.n_out);
    return csi_load_weights(c, model, t.data(), (int)t.size());
}

std::vector<WBlob> held(csi_ctx* c) {
    WireMeta w;
    wire_fill(c, w);
    std::vector<WBlob> b;
    wire_blobs(c, w, b);
    return b;
}

}  // namespace

int main() {
    const Shape shapes[3] = {{4, 2, {40, 24, 0}, 52, CSI_DTYPE_F32, 0}, {4, 2, {40, 24, 0}, 52, CSI_DTYPE_BF16, 0}, {4, 1, {24, 0, 0}, 20, CSI_DTYPE_F32, 1}};
    const size_t want_blobs[3] = {2 * 19, 2 * 12, 2 * 12};
    csi_destroy(make_ctx(shapes[0]));      // whatever the process allocates once and keeps is allocated now
    const long live0 = mock::g_live;
    size_t bytes = 0;
    for (int k = 0; k < 3; ++k) {
        csi_ctx *a = make_ctx(shapes[k]), *b = make_ctx(shapes[k]);
        const long empty = mock::g_live;
        for (int d = 0; d < 2; ++d) {
            const int rc = load(a, shapes[k], d, 17u + (unsigned)d);
            EXPECT(rc == CSI_OK && !*csi_last_error(a), "shape %d model %d: load rc %d (%s)", k, d, rc, csi_last_error(a));
        }
        EXPECT(csi_clone_weights(b, a) == CSI_OK, "shape %d: clone: %s", k, csi_last_error(b));
        const std::vector<WBlob> ha = held(a), hb = held(b);
        EXPECT(ha.size() == want_blobs[k] && hb.size() == ha.size(), "shape %d: %zu buffers on the source, %zu on the clone, %zu expected", k, ha.size(), hb.size(), want_blobs[k]);
        for (size_t i = 0; i < ha.size() && i < hb.size(); ++i) {
            EXPECT(ha[i].bytes == hb[i].bytes && *ha[i].p != *hb[i].p && !std::memcmp(*ha[i].p, *hb[i].p, ha[i].bytes), "shape %d: buffer %zu differs on the clone", k, i);
            bytes += ha[i].bytes;
        }
        EXPECT(load(a, shapes[k], 0, 99u) == CSI_OK, "shape %d: reload: %s", k, csi_last_error(a));      // a load over a loaded model frees what it replaces
        EXPECT(mock::g_live - empty >= (long)(ha.size() + hb.size()), "shape %d: %ld buffers alive for %zu blobs", k, mock::g_live - empty, ha.size() + hb.size());
        csi_destroy(a);
        csi_destroy(b);
        EXPECT(mock::g_live == live0, "shape %d: %ld device buffers left behind", k, mock::g_live - live0);
    }
    if (bad) std::printf("FAILED (%d)\n", bad);
    else std::printf("weights_check: ok  (3 shapes loaded, cloned, reloaded and destroyed; %zu bytes compared)\n", bytes);
    return bad != 0;
}
#endif
