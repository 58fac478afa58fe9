#define CIAO_T float
#include "gram_launch.inc"
