// tests/cpp/record_test.cpp — the record_data callback of emba_host::solveTimeWindow (emba_amd/host/solve_time_window.hpp) and
// emba_host::ShardedLEGM::render_map_images on the GPU.  At every record point it renders the four images and downloads the map; with an output
// directory it writes them as raw files rec_<n>.{gx,gy,rgb,poisson} (uint8) and rec_<n>.map (Gx then Gy, float64) for tests/test_cpp_record.py.
// Prints "REC <n> <iter> <final> <fnv1a of the four images>" per record point, then the LM log.
// Usage: record_test <in.bin> <devices> <max_iter> [out_dir]      (file layout: tests/cpp/host_test.cpp's)
#include "../../emba_amd/host/solve_time_window.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

template <class T> static std::vector<T> rd(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }
template <class T> static T rd1(FILE* f) { return rd<T>(f, 1)[0]; }

static uint64_t fnv1a(const std::vector<uint8_t>& v, uint64_t h = 0xCBF29CE484222325ull)
{
    for (uint8_t b : v) { h ^= b; h *= 0x100000001B3ull; }
    return h;
}

template <class T> static void wr(const std::string& path, const std::vector<T>& v)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(3); }
    fclose(f);
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int> devices;
    for (char* tok = strtok(argv[2], ","); tok; tok = strtok(nullptr, ",")) devices.push_back(atoi(tok));
    const int max_iter = atoi(argv[3]);
    const std::string out_dir = argc > 4 ? argv[4] : "";
    const int sw = rd1<int32_t>(f), sh = rd1<int32_t>(f), W = rd1<int32_t>(f), H = rd1<int32_t>(f), K = rd1<int32_t>(f), thres = rd1<int32_t>(f);
    const int64_t t0 = rd1<int64_t>(f), dt = rd1<int64_t>(f), n = rd1<int64_t>(f);
    const double C_th = rd1<double>(f), alpha = rd1<double>(f);
    auto lut = rd<double>(f, (size_t)sw * sh * 3); auto knots = rd<double>(f, (size_t)K * 4);
    auto gx = rd<double>(f, (size_t)W * H); auto gy = rd<double>(f, (size_t)W * H);
    auto x = rd<uint16_t>(f, n); auto y = rd<uint16_t>(f, n); auto pol = rd<uint8_t>(f, n); auto t = rd<int64_t>(f, n);
    fclose(f);
    emba_host::EventPacket ev(n);
    for (int64_t k = 0; k < n; ++k) ev[k] = {x[k], y[k], t[k], pol[k] != 0};
    try {
        emba_host::ShardedLEGM model(sw, sh, lut.data(), C_th, W, H, devices);
        emba_host::BASettings ba;
        ba.thres_valid_pixel = thres; ba.alpha = alpha;
        emba_host::LMSettings lm; lm.max_num_iter = max_iter;
        emba_host::TrajectoryView traj{knots.data(), K, t0, dt};
        const size_t np = (size_t)W * H;
        std::vector<uint8_t> ix(np), iy(np), irgb(3 * np), ip(np);
        std::vector<double> map(2 * np);
        int n_rec = 0;
        auto record = [&](int iter, bool final) {
            model.render_map_images(0.1, ix.data(), iy.data(), irgb.data(), ip.data());
            uint64_t h = fnv1a(ix); h = fnv1a(iy, h); h = fnv1a(irgb, h); h = fnv1a(ip, h);
            printf("REC %d %d %d %016llx\n", n_rec, iter, final ? 1 : 0, (unsigned long long)h);
            if (!out_dir.empty()) {
                model.downloadMap(map.data(), map.data() + np);
                const std::string b = out_dir + "/rec_" + std::to_string(n_rec);
                wr(b + ".gx", ix); wr(b + ".gy", iy); wr(b + ".rgb", irgb); wr(b + ".poisson", ip); wr(b + ".map", map);
            }
            ++n_rec;
        };
        const emba_host::LMResult r = emba_host::solveTimeWindow(model, traj, ev, gx.data(), gy.data(), ba, lm, nullptr, record);
        for (const auto& e : r.log) printf("LM %d %.1f %.17g %.17g %d\n", e.iter, e.log10_lambda, e.cost_min, e.cost_new, e.accepted ? 1 : 0);
        printf("END %d %d %.17g\n", r.iterations, r.converged ? 1 : 0, r.cost_min);
    } catch (const std::exception& e) { printf("FAIL exception %s\n", e.what()); return 1; }
    return 0;
}
