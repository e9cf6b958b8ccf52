/* A compress through Grok's public C API (include/grk_abi.h) of an image that carries a colour
 * description: what FileFormatCompress::initCompress reads from the grk_image.
 *   grk_api_encode_colour in.raw w h out mode fmt
 * in.raw holds int32 samples, plane after plane, 8 bits deep.
 * mode rgba: four components, sRGB, comps[3].type = GRK_COMPONENT_TYPE_OPACITY (whole image);
 * mode sycc: three components, GRK_CLRSPC_SYCC, with the MCT asked for (Grok clears it);
 * mode cie: three components, GRK_CLRSPC_DEFAULT_CIE (what Grok's TIFF reader sets for CIELab), a
 * colour space no JP2 box is written for here but which a raw codestream does not care about;
 * fmt jp2 | j2k.  Three resolutions, everything else as grk_compress_set_default_params leaves it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "grk_abi.h"

static void on_msg(const char* msg, void* ud) { (void)ud; fprintf(stderr, "%s\n", msg); }

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    const uint32_t w = (uint32_t)atoi(argv[2]), h = (uint32_t)atoi(argv[3]);
    const int rgba = !strcmp(argv[5], "rgba");
    const uint16_t c = rgba ? 4 : 3;
    const GRK_CODEC_FORMAT fmt = !strcmp(argv[6], "jp2") ? GRK_CODEC_JP2 : GRK_CODEC_J2K;
    grk_cparameters p;
    grk_compress_set_default_params(&p);
    p.numresolution = 3;
    p.mct = 1;
    grk_initialize(NULL, 0);
    grk_image_cmptparm cp[4];
    memset(cp, 0, sizeof cp);
    for (uint16_t k = 0; k < c; ++k) { cp[k].dx = cp[k].dy = 1; cp[k].prec = 8; cp[k].w = w; cp[k].h = h; }
    const GRK_COLOR_SPACE space = rgba ? GRK_CLRSPC_SRGB : !strcmp(argv[5], "cie") ? GRK_CLRSPC_DEFAULT_CIE : GRK_CLRSPC_SYCC;
    grk_image* img = grk_image_new(c, cp, space, true);
    if (!img) return 3;
    if (rgba) {
        img->comps[3].type = GRK_COMPONENT_TYPE_OPACITY;
        img->comps[3].association = GRK_COMPONENT_ASSOC_WHOLE_IMAGE;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 4;
    for (uint16_t k = 0; k < c; ++k)
        for (uint32_t y = 0; y < h; ++y)
            if (fread(img->comps[k].data + (size_t)y * img->comps[k].stride, 4, w, f) != w) return 5;
    fclose(f);
    grk_stream* st = grk_stream_create_file_stream(argv[4], 1024 * 1024, false);
    if (!st) return 6;
    grk_codec* codec = grk_compress_create(fmt, st);
    if (!codec) return 7;
    grk_set_warning_handler(on_msg, NULL);
    grk_set_error_handler(on_msg, NULL);
    if (!grk_compress_init(codec, &p, img) || !grk_compress_start(codec)) return 8;
    if (!grk_compress_with_plugin(codec, NULL) || !grk_compress_end(codec)) return 9;
    grk_object_unref(codec);
    grk_object_unref(st);
    grk_object_unref(&img->obj);
    grk_deinitialize();
    return 0;
}
