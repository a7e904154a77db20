// trails_host.cc — the host side of today's path, for tools/mapmaker/time_trails.py: Tracker::TrailTracking_Advance
// (src/Tracker.cc:376-432) with MiniPatch::FindPatch / SSDAtPoint (src/ImageProcess.cc:57-80, 204-252) restated in plain C++ on
// level-0 frames (image + FAST corners) read from a file, one thread, -O2.  Prints per frame "nGood nAlive microseconds".
//   in: int32 w, h, n_frames, n_trails | n_trails x (x, y) int32 | per frame: w * h bytes, int32 n_corners, n_corners x (x, y) int32
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <list>
#include <vector>

struct Ref {
    int32_t x, y;
};
struct Frame {
    std::vector<uint8_t> im;
    std::vector<Ref> corners;
};
struct Trail {
    uint8_t patch[81];
    Ref initial, current;
};
static int W, H;

static void sample(const Frame& f, Ref p, uint8_t* out) {
    for (int r = 0; r < 9; r++) std::memcpy(out + 9 * r, &f.im[(size_t)(p.y - 4 + r) * W + p.x - 4], 9);
}
static int ssd_at_point(const Frame& f, Ref p, const uint8_t* t, int max_ssd) {
    if (!(p.x >= 4 && p.y >= 4 && p.x < W - 4 && p.y < H - 4)) return max_ssd + 1;
    int s = 0;
    for (int r = 0; r < 9; r++) {
        const uint8_t* im = &f.im[(size_t)(p.y - 4 + r) * W + p.x - 4];
        for (int c = 0; c < 9; c++) {
            const int d = im[c] - t[9 * r + c];
            s += d * d;
        }
    }
    return s;
}
static bool find_patch(Ref& pos, const Frame& f, const uint8_t* t, int range = 10, int max_ssd = 100000) {
    Ref best{0, 0};
    int best_ssd = max_ssd + 1;
    const Ref tl{pos.x - range, pos.y - range}, br{pos.x + range, pos.y + range};
    auto i = f.corners.begin();
    for (; i != f.corners.end(); i++)
        if (i->y >= tl.y) break;
    for (; i != f.corners.end(); i++) {
        if (i->x < tl.x || i->x > br.x) continue;
        if (i->y > br.y) break;
        const int s = ssd_at_point(f, *i, t, max_ssd);
        if (s < best_ssd) best = *i, best_ssd = s;
    }
    if (best_ssd < max_ssd) {
        pos = best;
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fp = std::fopen(argv[1], "rb");
    int32_t h[4];
    if (!fp || std::fread(h, 4, 4, fp) != 4) return 3;
    W = h[0], H = h[1];
    std::vector<Ref> starts((size_t)h[3]);
    if (std::fread(starts.data(), sizeof(Ref), starts.size(), fp) != starts.size()) return 3;
    std::vector<Frame> frames((size_t)h[2]);
    for (Frame& f : frames) {
        f.im.resize((size_t)W * H);
        int32_t n;
        if (std::fread(f.im.data(), 1, f.im.size(), fp) != f.im.size() || std::fread(&n, 4, 1, fp) != 1) return 3;
        f.corners.resize((size_t)n);
        if (n && std::fread(f.corners.data(), sizeof(Ref), (size_t)n, fp) != (size_t)n) return 3;
    }
    std::list<Trail> trails;
    for (Ref s : starts) {
        Trail t;
        sample(frames[0], s, t.patch);
        t.initial = t.current = s;
        trails.push_back(t);
    }
    for (size_t k = 1; k < frames.size(); k++) {
        const auto t0 = std::chrono::steady_clock::now();
        const Frame &cur = frames[k], &prev = frames[k - 1];
        int good = 0;
        for (auto i = trails.begin(); i != trails.end();) {
            const Ref start = i->current;
            Ref end = start;
            bool found = find_patch(end, cur, i->patch);
            if (found) {
                uint8_t back[81];
                sample(cur, end, back);
                Ref b = end;
                found = find_patch(b, prev, back);
                const int dx = b.x - start.x, dy = b.y - start.y;
                if (dx * dx + dy * dy > 2) found = false;
                i->current = end;
                good++;
            }
            i = found ? std::next(i) : trails.erase(i);
        }
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%d %zu %.1f\n", good, trails.size(), us);
    }
    return 0;
}
