/* lj_scaled.c -- IJG libjpeg 9's own reduced-size decode of a gray file, for
 * the pin of the 1x1 and 2x2 transforms (tests/test_lowres.py):
 *   lj_scaled IN.jpg NUM OUT.raw
 * decodes IN.jpg with scale_num = NUM, scale_denom = 8, JDCT_ISLOW to
 * JCS_GRAYSCALE, writes the samples row by row to OUT.raw and prints
 * "width height".  Linked against libjpeg.so.9 as oracle/Makefile links ljpin. */
#include <stdio.h>
#include <stdlib.h>

#include <jpeglib.h>

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: lj_scaled IN.jpg NUM OUT.raw\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  struct jpeg_decompress_struct cinfo;
  struct jpeg_error_mgr jerr;
  cinfo.err = jpeg_std_error(&jerr);
  jpeg_create_decompress(&cinfo);
  jpeg_stdio_src(&cinfo, in);
  jpeg_read_header(&cinfo, TRUE);
  cinfo.scale_num = (unsigned)atoi(argv[2]);
  cinfo.scale_denom = 8;
  cinfo.dct_method = JDCT_ISLOW;
  cinfo.out_color_space = JCS_GRAYSCALE;
  jpeg_start_decompress(&cinfo);
  JSAMPLE* row = (JSAMPLE*)malloc(cinfo.output_width);
  if (!row) return 2;
  while (cinfo.output_scanline < cinfo.output_height) {
    JSAMPROW rows[1] = {row};
    jpeg_read_scanlines(&cinfo, rows, 1);
    fwrite(row, 1, cinfo.output_width, out);
  }
  printf("%u %u\n", cinfo.output_width, cinfo.output_height);
  jpeg_finish_decompress(&cinfo);
  jpeg_destroy_decompress(&cinfo);
  free(row);
  fclose(in);
  fclose(out);
  return 0;
}
