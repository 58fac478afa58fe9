#include "gramcd_launch.inc"
