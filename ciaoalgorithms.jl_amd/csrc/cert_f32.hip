#define CIAO_T float
#include "cert_launch.inc"
