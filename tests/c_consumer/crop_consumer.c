/* A plain C99 consumer of the cropped decode's declarations in include/compeg_hip.h (test infrastructure), compiled with
 * gcc -std=c99 -Wall -Wextra -Werror -pedantic and linked against libcompeg_hip.so by tests/test_crop_stream.py.  No
 * device: compeg_crop_shape alone is called; the decode entry points are named, so that their declarations are used.
 *   crop_consumer W H x y w h format pitch    prints "shape PITCH TOTAL", or "refused CODE: message" */
#include <stdio.h>
#include <stdlib.h>

#include "compeg_hip.h"

typedef int (*batch_fn)(compeg_batch *, const compeg_crop_spec *, void *, size_t, void *);
typedef int (*decoder_fn)(compeg_decoder *, const compeg_image *, const compeg_crop_spec *, void *, size_t, void *);
typedef int (*blocking_fn)(compeg_decoder *, const compeg_image *, const compeg_crop_spec *, void *, size_t);

int main(int argc, char **argv)
{
    const batch_fn batch = compeg_batch_decode_cropped;
    const decoder_fn decoder = compeg_decoder_decode_cropped;
    const blocking_fn blocking = compeg_decoder_decode_cropped_blocking;
    compeg_crop_spec spec = {0, 0, 0, 0, COMPEG_CROP_RGBA, 0, {0, 0}};
    uint32_t pitch = 0;
    uint64_t total = 0;
    int rc;
    if (argc != 9 || !batch || !decoder || !blocking || sizeof spec != 32 || COMPEG_KERNEL_CROPPED != 11 || COMPEG_CROP_RGB_PLANAR != 1)
        return 2;
    spec.x = (uint32_t)atoi(argv[3]);
    spec.y = (uint32_t)atoi(argv[4]);
    spec.width = (uint32_t)atoi(argv[5]);
    spec.height = (uint32_t)atoi(argv[6]);
    spec.format = (uint32_t)atoi(argv[7]);
    spec.pitch = (uint32_t)atoi(argv[8]);
    rc = compeg_crop_shape(&spec, (uint32_t)atoi(argv[1]), (uint32_t)atoi(argv[2]), &pitch, &total);
    if (rc != COMPEG_OK) {
        printf("refused %d: %s\n", rc, compeg_last_error());
        return 0;
    }
    printf("shape %u %llu\n", pitch, (unsigned long long)total);
    return 0;
}
