// isvc_layout_probe.cpp - prints the sizes, offsets and enumerator values of the ISVCDecoder interface that a client's binary
// depends on.  Built with -DLH264_PROBE_HEADER='"lh264_isvc.h"' by tests/test_isvc.py and with '"codec_api.h"' (the reference's
// own header) by oracle/Makefile into oracle/_ref/isvc_layout_refhdr.txt; both must print LAYOUT_EXPECTED of tests/test_isvc.py.
#include <stdio.h>
#include <stddef.h>
#include LH264_PROBE_HEADER
int main() {
  printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(SDecodingParam), sizeof(SBufferInfo), sizeof(SSysMEMBuffer), sizeof(SDecoderCapability),
         sizeof(SParserBsInfo), sizeof(SDecoderStatistics), sizeof(OpenH264Version));
  printf("%zu %zu %zu %zu %zu %zu ", offsetof(SDecodingParam, eOutputColorFormat), offsetof(SDecodingParam, uiTargetDqLayer),
         offsetof(SDecodingParam, eEcActiveIdc), offsetof(SDecodingParam, bParseOnly), offsetof(SDecodingParam, sVideoProperty),
         offsetof(SBufferInfo, UsrData));
  printf("%zu %zu %zu ", offsetof(SBufferInfo, uiOutYuvTimeStamp), offsetof(SParserBsInfo, pDstBuff), offsetof(SDecoderStatistics, iAvgLumaQp));
  printf("%d %d %d %d %d %d %d\n", (int)dsInitialOptExpected, (int)dsDstBufNeedExpan, (int)DECODER_OPTION_GET_STATISTICS,
         (int)ERROR_CON_SLICE_MV_COPY_CROSS_IDR_FREEZE_RES_CHANGE, (int)videoFormatI420, (int)cmUnsupportedData, (int)FEEDBACK_UNKNOWN_NAL);
  return 0;
}
