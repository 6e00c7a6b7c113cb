// Print, from the plan functions of scarlet_amd/csrc/launch_plan.h, the frame sides at which each form begins (the
// table of DESIGN.md "One plan").  Host code only, no GPU needed:
//     hipcc --offload-arch=gfx950 -O1 -std=c++17 -Iinclude tools/native/launch_forms.hip -o launch_forms && ./launch_forms
#include <stdio.h>
#include "../../scarlet_amd/csrc/launch_plan.h"

__constant__ unsigned short sc_nfl_table[SC_NFL_MAX];       // (the kernels of the headers link against it; never launched)

int main(void)
{
    const UpdateWants wants = {true, true, true, true, true};
    const char *const forms[] = {"wave", "<0> tile and scratch in LDS", "<1> tile in LDS, scratch in HBM", "<2> plane in HBM"};
    const char *const boxes[] = {"none", "<0,0> streamed", "<8,128>", "<16,256>", "<8,0>", "<16,0>"};
    int form = -1, box = -1, scratch = -1, init_lds = -1;
    size_t box_max = 0;
    printf("square frames, sides 4, 8 .. %d (monotonic batch, default switches)\n", SCARLET_MAX_SIDE);
    for (int n = 4; n <= SCARLET_MAX_SIDE; n += 4) {
        const UpdatePlan p = update_plan(n, n, wants);
        const InitTilePlan t = init_tile_plan(n, n, 1);
        if (p.form != form) printf("side %4d: update form %s, %zu bytes of LDS\n", n, forms[form = p.form], p.lds);
        if ((int)p.reserve_gscratch != scratch) printf("side %4d: workspace %s gscratch\n", n, (scratch = p.reserve_gscratch) ? "reserves" : "has no");
        if (p.box != box || n == 128 || n == 132 || n == 256 || n == 260)
            printf("side %4d: box %s, %zu and %zu bytes of LDS (update: %zu)\n", n, boxes[box = p.box], p.box_lds[0], p.box_lds[1], p.lds);
        if ((int)t.in_lds != init_lds) printf("side %4d: float64 initialisation tile in %s\n", n, (init_lds = t.in_lds) ? "LDS" : "HBM");
        if (n > 64 && p.box == BOX_NONE) printf("side %4d: the box does not fit LDS\n", n);
        if (p.box_lds[1] > box_max) box_max = p.box_lds[1];
    }
    for (int n = 1; n <= SCARLET_MAX_SIDE; ++n)      // every side, for the first float64 tile that leaves LDS
        if (!init_tile_plan(n, n, 1).in_lds) { printf("side %4d: first float64 initialisation tile in HBM (every side counted)\n", n); break; }
    printf("largest 127 x 127 box: %zu bytes (LDS_LIMIT %zu)\n", box_max, LDS_LIMIT);
    // every shape up to SCARLET_MAX_SIDE: the forms that take the scratch from the workspace find it reserved, and the
    // box fits
    long bad = 0, nobox = 0, spare = 0;
    int spare_h = 0, spare_w = 0;
    for (int h = 1; h <= SCARLET_MAX_SIDE; ++h)
        for (int w = 1; w <= SCARLET_MAX_SIDE; ++w) {
            const UpdatePlan p = update_plan(h, w, wants);
            bad += (p.form == FORM_TILE_GSCRATCH || p.form == FORM_PLANE) && !p.reserve_gscratch;
            nobox += (h > 64 || w > 64) && p.box == BOX_NONE;
            if (p.form == FORM_TILE && p.reserve_gscratch && !spare++) { spare_h = h; spare_w = w; }
        }
    printf("%ld shapes reserve gscratch and run <0> (the first: %d x %d)\n", spare, spare_h, spare_w);
    printf("all %d x %d shapes: %ld take HBM scratch the layout does not reserve, %ld beyond the wave tile have no box\n",
           SCARLET_MAX_SIDE, SCARLET_MAX_SIDE, bad, nobox);
    return bad != 0;
}
