#define CIAO_T double
#include "gram_launch.inc"
