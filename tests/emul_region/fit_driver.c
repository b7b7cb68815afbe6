/* Every compeg_region_fit(sw, sh, ow, oh) with all four extents in 1..N, both placements, against a table made by the
 * test (tests/test_region_api.py) -- built there with gcc and linked with the library; no device is touched.
 *
 *   fit_driver N TABLE
 *
 * TABLE: N^4 entries of four bytes (dx, dy, dw, dh), the centred placement, sw slowest and oh fastest.  The top-left
 * placement must give (0, 0, dw, dh) of the same entry.  Prints the number of calls that differ and the first one. */
#include <stdio.h>
#include <stdlib.h>

#include "compeg_hip.h"

int main(int argc, char **argv)
{
    unsigned n, sw, sh, ow, oh;
    unsigned long wrong = 0, calls = 0;
    size_t entries;
    unsigned char *table, *e;
    FILE *f;
    if (argc != 3 || (n = (unsigned)atoi(argv[1])) == 0 || n > 255) {
        fprintf(stderr, "usage: fit_driver N TABLE\n");
        return 2;
    }
    entries = (size_t)n * n * n * n;
    table = malloc(entries * 4);
    f = fopen(argv[2], "rb");
    if (!table || !f || fread(table, 4, entries, f) != entries) {
        fprintf(stderr, "fit_driver: cannot read the table\n");
        return 2;
    }
    fclose(f);
    e = table;
    for (sw = 1; sw <= n; sw++)
        for (sh = 1; sh <= n; sh++)
            for (ow = 1; ow <= n; ow++)
                for (oh = 1; oh <= n; oh++, e += 4) {
                    compeg_rect c = {77, 77, 77, 77}, t = {77, 77, 77, 77};
                    const int rc = compeg_region_fit(sw, sh, ow, oh, COMPEG_FIT_CENTER, &c);
                    const int rt = compeg_region_fit(sw, sh, ow, oh, COMPEG_FIT_TOP_LEFT, &t);
                    const int bad = rc != COMPEG_OK || rt != COMPEG_OK || c.x != e[0] || c.y != e[1] || c.width != e[2] || c.height != e[3] ||
                                    t.x != 0 || t.y != 0 || t.width != e[2] || t.height != e[3];
                    calls += 2;
                    if (bad && wrong++ == 0)
                        printf("first %ux%u into %ux%u: centred (%u, %u, %u, %u), top-left (%u, %u, %u, %u), expected (%u, %u, %u, %u)\n", sw, sh, ow, oh,
                               c.x, c.y, c.width, c.height, t.x, t.y, t.width, t.height, e[0], e[1], e[2], e[3]);
                }
    printf("calls %lu wrong %lu\n", calls, wrong);
    free(table);
    return wrong ? 1 : 0;
}
