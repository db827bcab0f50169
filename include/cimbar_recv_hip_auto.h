/* cimbar_recv_hip_auto.h -- one symbol of libcimbar_recv_hip.so beside the reference's (include/cimbar_recv_hip.h): the web receiver's auto mode.
 *
 * cimbard_hip_scan_extract_decode_auto(img, w, h, format, bufspace, bufsize, mode_out)
 *     what web/recv.js does per camera frame in auto mode (recv.js:112,346,378), in one call: cimbard_configure_decode(m) +
 *     cimbard_scan_extract_decode for m = 66, 68, 67, 4 in turn until one returns bytes, with ONE carried colour-correction matrix shared by the
 *     four modes (per calling thread, like the reference's CimbDecoder.cpp:69-73). Returns what cimbard_scan_extract_decode returns for the
 *     accepted mode (bytes packed front to back, *mode_out = the mode), 0 with *mode_out = 0 where no mode delivered a chunk, -1 for an empty
 *     image, -2 if bufsize is smaller than the largest of the four modes' cimbard_get_bufsize (7500), -3 if no frame was found and -4 if the GPU
 *     path failed (cimbard_get_report holds the message). cimbard_configure_decode does not affect it, nor it the mode that call selected.
 */
#ifndef CIMBAR_RECV_HIP_AUTO_H
#define CIMBAR_RECV_HIP_AUTO_H

#ifdef __cplusplus
extern "C" {
#endif

int cimbard_hip_scan_extract_decode_auto(const unsigned char* imgdata, unsigned imgw, unsigned imgh, int format, unsigned char* bufspace,
                                         unsigned bufsize, int* mode_out);

#ifdef __cplusplus
}
#endif
#endif /* CIMBAR_RECV_HIP_AUTO_H */
