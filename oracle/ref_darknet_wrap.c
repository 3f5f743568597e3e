// ref_darknet_wrap.c - thin C wrapper (this repo's own code) around the REAL darknet of the reference
// (Thirdparty/darknet/src/*.c, compiled where it lies by oracle/Makefile.ref, CPU only, -ffp-contract=off).
// TEST INFRASTRUCTURE ONLY: the compiled-reference oracle for the device detector (svo_det_*) and for its numpy
// restatement (tests/darknet_ref.py).  The reference's own entry points YoloLoad and YoloDetectFromImage are exported by
// the library as they are; this file adds what YoloDetectFromImage hides:
//  ref_dn_net_size / ref_dn_layer_info : the network's input size and layer count; darknet's own shape of every layer and its
//                                        parameter count
//  ref_dn_layer_type_ids               : this build's LAYER_TYPE values of the layer types the device supports
//  ref_dn_forward                      : network_predict on a ready network input
//  ref_dn_layer_output                 : pointer + size of a layer's `output` after a forward
//  ref_dn_letterbox                    : letterbox_image on a planar float image
//  ref_dn_flush                        : fflush of stdout and stderr (the loader silences darknet's layer table)
//  ref_dn_free                         : free_network
// No reference source is modified or copied.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "darknet.h"

int ref_dn_net_size(int* _net, int32_t* whc) {
  network* net = (network*)_net;
  whc[0] = net->w; whc[1] = net->h; whc[2] = net->c;
  return net->n;
}

// info[0..8] = type (darknet's LAYER_TYPE), w, h, c, out_w, out_h, out_c, outputs, parameter floats read by load_weights
int ref_dn_layer_info(int* _net, int i, int32_t* info) {
  network* net = (network*)_net;
  if (i < 0 || i >= net->n) return -1;
  layer l = net->layers[i];
  info[0] = (int32_t)l.type;
  info[1] = l.w; info[2] = l.h; info[3] = l.c;
  info[4] = l.out_w; info[5] = l.out_h; info[6] = l.out_c;
  info[7] = l.outputs;
  info[8] = 0;
  if (l.type == CONVOLUTIONAL) info[8] = l.n * (l.batch_normalize ? 4 : 1) + l.nweights;
  return 0;
}

int ref_dn_layer_type_ids(int32_t* ids) {   // the enum values this build gives the types the device supports
  ids[0] = CONVOLUTIONAL; ids[1] = MAXPOOL; ids[2] = ROUTE; ids[3] = SHORTCUT; ids[4] = UPSAMPLE; ids[5] = YOLO; ids[6] = REGION;
  return 7;
}

void ref_dn_forward(int* _net, float* input) { network_predict((network*)_net, input); }

int ref_dn_layer_output(int* _net, int i, float** out) {
  network* net = (network*)_net;
  if (i < 0 || i >= net->n) return -1;
  *out = net->layers[i].output;
  return net->layers[i].outputs;
}

// letterbox_image of a planar float image (c x h x w) into out (c x nh x nw)
void ref_dn_letterbox(float* data, int w, int h, int c, int nw, int nh, float* out) {
  image im;
  im.data = data; im.w = w; im.h = h; im.c = c;
  image s = letterbox_image(im, nw, nh);
  memcpy(out, s.data, sizeof(float) * (size_t)nw * nh * c);
  free_image(s);
}

void ref_dn_flush(void) { fflush(stdout); fflush(stderr); }

void ref_dn_free(int* _net) { free_network((network*)_net); }
