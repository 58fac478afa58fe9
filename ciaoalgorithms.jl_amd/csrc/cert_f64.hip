#define CIAO_T double
#include "cert_launch.inc"
