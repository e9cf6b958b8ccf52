/* A decompress through Grok's public C API (include/grk_abi.h) that reports what the library
 * makes of a JP2 file's colour boxes: the composited image after grk_decompress_read_header
 * (the codestream's components, colour space, ICC profile) and the same object after
 * grk_decompress (FileFormatDecompress::applyColour: palette channels, cdef order and types).
 *   grk_api_colour in.jp2 out.raw [icc.bin]
 * out.raw receives the int32 samples of every component, plane after plane. */
#include <stdio.h>
#include <string.h>
#include "grk_abi.h"

static void on_msg(const char* msg, void* ud) { (void)ud; fprintf(stderr, "%s\n", msg); }

static void show(const char* tag, const grk_image* img) {
    printf("%s comps %u space %d applied %d icc %u\n", tag, img->numcomps, (int)img->color_space, (int)img->color_applied,
           img->meta ? img->meta->color.icc_profile_len : 0u);
    for (uint32_t k = 0; k < img->numcomps; ++k)
        printf("%s comp %u prec %u sgnd %d type %u assoc %u\n", tag, k, img->comps[k].prec, (int)img->comps[k].sgnd,
               (unsigned)img->comps[k].type, (unsigned)img->comps[k].association);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    grk_decompress_parameters params;
    memset(&params, 0, sizeof params);
    grk_decompress_set_default_params(&params.core);
    grk_initialize(NULL, 0);
    grk_stream* st = grk_stream_create_file_stream(argv[1], 1024 * 1024, true);
    if (!st) return 3;
    grk_codec* codec = grk_decompress_create(GRK_CODEC_JP2, st);
    if (!codec) return 4;
    grk_set_warning_handler(on_msg, NULL);
    grk_set_error_handler(on_msg, NULL);
    if (!grk_decompress_init(codec, &params.core)) return 5;
    if (!grk_decompress_read_header(codec, NULL)) return 6;
    grk_image* img = grk_decompress_get_composited_image(codec);
    if (!img) return 7;
    show("header", img);
    if (argc > 3 && img->meta && img->meta->color.icc_profile_len) {
        FILE* g = fopen(argv[3], "wb");
        fwrite(img->meta->color.icc_profile_buf, 1, img->meta->color.icc_profile_len, g);
        fclose(g);
    }
    if (!grk_decompress_set_window(codec, 0, 0, 0, 0)) return 8;
    if (!(grk_decompress(codec, NULL) && grk_decompress_end(codec))) return 9;
    if (grk_decompress_get_composited_image(codec) != img) return 10;   /* the same object, edited in place */
    show("image", img);
    FILE* f = fopen(argv[2], "wb");
    for (uint32_t k = 0; k < img->numcomps; ++k)
        for (uint32_t y = 0; y < img->comps[k].h; ++y)
            fwrite(img->comps[k].data + (size_t)y * img->comps[k].stride, 4, img->comps[k].w, f);
    fclose(f);
    grk_object_unref(st);
    grk_object_unref(codec);
    grk_deinitialize();
    return 0;
}
