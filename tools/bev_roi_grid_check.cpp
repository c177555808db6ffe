// bev_roi_grid_check.cpp -- csrc/bev_roi_grid.h on the host, under the sanitizers, on a table of hostile positions.
//
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=undefined,address -fsanitize=float-cast-overflow \
//       -fno-sanitize-recover=all tools/bev_roi_grid_check.cpp -o build/bev_roi_grid_check && build/bev_roi_grid_check
//
// Runs on the CPU only.  Every position of the table goes through bev_roi_corners against a small map; a corner it
// hands out is then READ from a heap plane of exactly h * w floats, so an index one past the map is an AddressSanitizer
// report, and a float -> int conversion of a value that does not fit is an UndefinedBehaviorSanitizer report.  Hostile
// RoI rows (NaN, infinity, 1e30) go through the theta and position expressions as well.  Exit status 0: every row behaved.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../pdanet_amd/csrc/bev_roi_grid.h"

static int failures = 0;

#define EXPECT(cond, ...)                  \
    do {                                   \
        if (!(cond)) {                     \
            ++failures;                    \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");             \
        }                                  \
    } while (0)

// the sample at (ix, iy) of a plane that holds 1 everywhere: the sum of the weights of the corners inside the map
static float sample_ones(const std::vector<float>& plane, float ix, float iy, int w, int h, bool& live, int& corners) {
    pda::BevCorners c;
    live = pda::bev_roi_corners(ix, iy, w, h, c);
    float acc = 0.f;
    corners = 0;
    for (int k = 0; k < 4; ++k) {
        if (c.off[k] >= 0) {
            acc += c.wt[k] * plane.data()[c.off[k]];   // an index outside the heap block is an ASan report
            ++corners;
        }
        if (!live) EXPECT(c.off[k] == -1 && c.wt[k] == 0.f, "dead sample (%g, %g) hands out corner %d", ix, iy, k);
    }
    return acc;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int w : {2, 9, 176}) {
        const int h = w == 9 ? 17 : (w == 2 ? 2 : 200);
        const std::vector<float> plane((size_t)h * w, 1.0f);
        const float fw = (float)w, fh = (float)h;
        struct Row { float pos; bool live; int corners_x; };   // corners_x: columns of the map the sample touches along this axis
        const std::vector<Row> table = {
            {nan, false, 0}, {-nan, false, 0}, {inf, false, 0}, {-inf, false, 0}, {1e30f, false, 0}, {-1e30f, false, 0},
            {3.4e38f, false, 0}, {-3.4e38f, false, 0}, {2147483648.0f, false, 0}, {-2147483904.0f, false, 0},
            {std::nextafterf(-1.0f, -2.0f), false, 0},
            {-1.0f, true, 1},                                  // floor -1: only the right column, weight 0
            {std::nextafterf(-1.0f, 0.0f), true, 1},           // -1 + one ulp
            {-0.5f, true, 1}, {-0.0f, true, 2}, {0.0f, true, 2}, {0.25f, true, 2},
            {fw - 2.0f, true, 2},
            {fw - 1.0f, true, 1},                              // floor w - 1: only the left column
            {fw - 0.5f, true, 1},
            {std::nextafterf(fw, 0.0f), true, 1},              // w minus one ulp
            {fw, false, 0}, {std::nextafterf(fw, 2 * fw), false, 0}, {fw + 1.0f, false, 0},
        };
        for (const Row& rx : table) {
            for (const Row& ry_src : table) {
                // the same table along y, scaled to the map's height where the entry is relative to the width
                Row ry = ry_src;
                if (ry.pos == fw - 2.0f) ry.pos = fh - 2.0f;
                else if (ry.pos == fw - 1.0f) ry.pos = fh - 1.0f;
                else if (ry.pos == fw - 0.5f) ry.pos = fh - 0.5f;
                else if (ry.pos == std::nextafterf(fw, 0.0f)) ry.pos = std::nextafterf(fh, 0.0f);
                else if (ry.pos == fw) ry.pos = fh;
                else if (ry.pos == std::nextafterf(fw, 2 * fw)) ry.pos = std::nextafterf(fh, 2 * fh);
                else if (ry.pos == fw + 1.0f) ry.pos = fh + 1.0f;
                bool live;
                int corners;
                const float got = sample_ones(plane, rx.pos, ry.pos, w, h, live, corners);
                const bool want_live = rx.live && ry.live;
                EXPECT(live == want_live, "w=%d h=%d (%g, %g): live %d, expected %d", w, h, rx.pos, ry.pos, (int)live, (int)want_live);
                if (want_live) {
                    EXPECT(corners == rx.corners_x * ry.corners_x, "w=%d h=%d (%g, %g): %d corners, expected %d", w, h, rx.pos,
                           ry.pos, corners, rx.corners_x * ry.corners_x);
                    EXPECT(got >= 0.f && got <= 1.0f, "w=%d h=%d (%g, %g): sample of ones %g", w, h, rx.pos, ry.pos, got);
                } else {
                    EXPECT(corners == 0 && got == 0.f, "w=%d h=%d (%g, %g): a dead sample read %d corners", w, h, rx.pos, ry.pos, corners);
                }
            }
        }
        // an interior position on the lattice is exact: (2.5, 1.25) -> weights .5 .5 x .75 .25
        if (w >= 9) {
            pda::BevCorners c;
            EXPECT(pda::bev_roi_corners(2.5f, 1.25f, w, h, c), "interior sample dead");
            EXPECT(c.off[0] == 1 * w + 2 && c.off[1] == 1 * w + 3 && c.off[2] == 2 * w + 2 && c.off[3] == 2 * w + 3, "interior offsets");
            EXPECT(c.wt[0] == 0.375f && c.wt[1] == 0.375f && c.wt[2] == 0.125f && c.wt[3] == 0.125f, "interior weights");
        }
        // RoI rows through theta and the positions, then through the corners.  The first ten are hostile in a way that
        // reaches every sample (a NaN, an infinity or 1e30 in the centre or the heading) and must read nothing; a huge SIZE
        // alone leaves the sample at u = v = 0 of an odd grid in the map, as it does in the reference.
        const float rows[][7] = {
            {nan, 1, 0, 2, 2, 1, 0}, {1, nan, 0, 2, 2, 1, 0}, {1, 1, 0, nan, 2, 1, 0}, {1, 1, 0, 2, 2, 1, nan},
            {inf, 1, 0, 2, 2, 1, 0}, {1, -inf, 0, 2, 2, 1, 0}, {1, 1, 0, inf, inf, 1, 0}, {inf, inf, inf, inf, inf, inf, 0},
            {1e30f, 1e30f, 1e30f, 1e30f, 1e30f, 1e30f, 0.3f}, {-1e30f, 1, 0, 2, 2, 1, 0}, {1, 1, 0, 1e30f, 2, 1, 1},
            {1e30f, 1e30f, 0, 1e38f, 1e38f, 1, 3.0f}, {0, 0, 0, 0, 0, 0, 0}, {3, 3, 0, 2, 1, 1, 0.7f},
        };
        int dead_first = 0, n_row = 0;
        for (const auto& row : rows) {
            const bool ok = pda::bev_finite_bits(row[6]);
            const float a = ok ? row[6] : 0.f;
            const pda::BevTheta th = pda::bev_roi_theta(row, std::cos(a), std::sin(a), w, h, 0.f, -1.f, 0.4f, 0.4f);
            bool any = false;
            for (int g : {1, 4, 7, 16})
                for (int i = 0; i < g; ++i)
                    for (int j = 0; j < g; ++j) {
                        float ix, iy;
                        pda::bev_roi_position(th, i, j, g, w, h, ix, iy);
                        if (!ok) ix = nan;
                        bool live;
                        int corners;
                        const float got = sample_ones(plane, ix, iy, w, h, live, corners);
                        EXPECT(got >= 0.f && got <= 1.0f, "row sample %g", got);
                        any = any || corners > 0;
                    }
            dead_first += (!any && n_row < 10) ? 1 : 0;
            ++n_row;
        }
        EXPECT(dead_first == 10, "w=%d: %d of the 10 hostile rows read nothing", w, dead_first);
    }
    if (failures) {
        std::printf("bev_roi_grid_check: %d failures\n", failures);
        return 1;
    }
    std::printf("bev_roi_grid_check: ok\n");
    return 0;
}
